"""Times the PCD codec (csrc/prh_pcd.hpp) against the host functions it replaces, in one run, and
writes profiles/r07_pcd_codec_bench.txt.

  format   pcd.format_rows on 250,000 rows, and on every slice of scripts/drive_slice_bench.py's
           drive at once (20 M points, 80 slices), against np.savetxt(fmt='%.4f %.4f %.4f %d')
  d2h      the one device -> host copy of that text
  parse    pcd.parse_rows on the same texts against np.loadtxt(dtype=float32)
  unpack   the 14-byte record kernel at 20 M points against load_pcd_data's numpy column_stack

Device times are HIP events around the call (format_rows and parse_rows include their prefix sum
and the read-back of the totals between the passes), one warm-up, median of --reps with all runs
listed.  Host times are wall clock, one thread; on the large text the host functions are timed on
the first slice and scaled by rows.  Algorithmic bytes: format = 2 passes x row bytes in + text out;
parse = 2 passes over the text + 1 parse pass + 4 B x columns out; the HBM figure is 8 TB/s.

    python scripts/pcd_codec_bench.py [--points 20000000] [--slices 80] [--out FILE]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
HBM_GBPS = 8000.0
FMT = "%.4f %.4f %.4f %d"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--slices", type=int, default=80)
    ap.add_argument("--rows", type=int, default=250_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_pcd_codec_bench.txt"))
    args = ap.parse_args()
    import torch
    from drive_slice_bench import make_drive
    from pointnet_refine_amd import drive, pcd
    if not torch.cuda.is_available():
        raise SystemExit("pcd_codec_bench.py needs a GPU")

    def device_ms(fn):
        fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keep = fn()
            e1.record()
            torch.cuda.synchronize()
            runs.append(round(e0.elapsed_time(e1), 3))
        return float(np.median(runs)), runs, keep

    def host_ms(fn, reps):
        fn()
        runs = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            runs.append(round((time.perf_counter() - t) * 1e3, 1))
        return float(np.median(runs)), runs

    def codec(points, offsets, host_rows, host_reps):
        """format / d2h / parse of points on the device; the host pair on host_rows of them."""
        n = points.shape[0]
        f_ms, f_runs, (text, boff) = device_ms(lambda: pcd.format_rows(points, offsets))
        nbytes = text.numel()
        c_ms, c_runs, _ = device_ms(lambda: text.cpu())
        p_ms, p_runs, vals = device_ms(lambda: pcd.parse_rows(text, 4))
        sub = points[:host_rows].cpu().numpy()
        buf = io.StringIO()
        np.savetxt(buf, sub, fmt=FMT)
        sub_text = buf.getvalue()
        assert sub_text.encode() == text[:len(sub_text)].cpu().numpy().tobytes()
        want = np.loadtxt(io.StringIO(sub_text), dtype=np.float32)
        assert np.array_equal(vals[:host_rows].cpu().numpy().view(np.int32), want.view(np.int32))
        s_ms, s_runs = host_ms(lambda: np.savetxt(io.StringIO(), sub, fmt=FMT), host_reps)
        l_ms, l_runs = host_ms(lambda: np.loadtxt(io.StringIO(sub_text), dtype=np.float32), host_reps)
        scale = n / host_rows
        f_bytes = 2 * points.element_size() * 4 * n + nbytes
        p_bytes = 3 * nbytes + 16 * n
        return {"rows": n, "text_bytes": nbytes, "format_ms": f_ms, "format_ms_all": f_runs,
                "format_gbps": round(f_bytes / f_ms / 1e6, 1), "format_hbm_fraction": round(f_bytes / f_ms / 1e6 / HBM_GBPS, 4),
                "d2h_ms": c_ms, "d2h_ms_all": c_runs, "d2h_gbps": round(nbytes / c_ms / 1e6, 1),
                "parse_ms": p_ms, "parse_ms_all": p_runs, "parse_gbps": round(p_bytes / p_ms / 1e6, 1),
                "parse_hbm_fraction": round(p_bytes / p_ms / 1e6 / HBM_GBPS, 4),
                "host_rows_timed": host_rows, "savetxt_ms": round(s_ms * scale, 1), "savetxt_ms_all": s_runs,
                "loadtxt_ms": round(l_ms * scale, 1), "loadtxt_ms_all": l_runs,
                "format_speedup": round(s_ms * scale / (f_ms + c_ms), 1), "parse_speedup": round(l_ms * scale / p_ms, 1)}

    dev = torch.device("cuda")
    cloud, poses, _ = make_drive(args.points, args.slices, 1)
    points, offsets, _ = drive.slice_cloud(torch.from_numpy(cloud).to(dev), poses)
    off = offsets.cpu().numpy()
    small = codec(points[:args.rows].contiguous(), None, args.rows, args.reps)
    large = codec(points, offsets, int(off[1] - off[0]), 1)
    del points

    rec = np.zeros(args.points, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<u2")]))
    rec["x"], rec["y"], rec["z"], rec["intensity"] = cloud[:, 0], cloud[:, 1], cloud[:, 2], cloud[:, 3].astype(np.uint16)
    payload = rec.tobytes()
    pay = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(dev)
    u_ms, u_runs, got = device_ms(lambda: pcd.unpack_records14(pay, args.points))

    def host_unpack():
        r = np.frombuffer(payload, dtype=rec.dtype)
        return np.column_stack((r["x"], r["y"], r["z"], r["intensity"].astype(np.float32)))

    assert np.array_equal(got.cpu().numpy().view(np.int32), host_unpack().view(np.int32))
    h_ms, h_runs = host_ms(host_unpack, args.reps)
    up_ms, up_runs, _ = device_ms(lambda: torch.from_numpy(cloud).to(dev))
    unpack = {"points": args.points, "unpack_ms": u_ms, "unpack_ms_all": u_runs,
              "unpack_gbps": round(30.0 * args.points / u_ms / 1e6, 1),
              "unpack_hbm_fraction": round(30.0 * args.points / u_ms / 1e6 / HBM_GBPS, 4),
              "host_column_stack_ms": h_ms, "host_column_stack_ms_all": h_runs,
              "upload_16B_per_point_ms": up_ms, "upload_ms_all": up_runs}
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows_250k": small, "drive_slices": large,
           "slices": args.slices, "unpack14": unpack}
    lines = ["PCD codec: pcd.format_rows / parse_rows / the 14-byte unpack against np.savetxt / np.loadtxt / numpy column_stack.",
             f"Command: python scripts/pcd_codec_bench.py --points {args.points} --slices {args.slices} --rows {args.rows} "
             f"--reps {args.reps}",
             "Timing: HIP events around each call (format_rows and parse_rows include torch.cumsum and the read-back of the",
             "totals between their passes), one warm-up, median of the listed runs; host functions by wall clock on one",
             "thread, on the large text timed on the first slice and scaled by rows.  Outputs compared in the run.",
             "Algorithmic bytes: format 2 x input + text; parse 3 x text + 16 B x rows; unpack 30 B x points; HBM 8 TB/s.",
             "", json.dumps(out), ""]
    for name, r in (("250 k rows", small), (f"{args.slices} slices of the drive", large)):
        lines += [f"{name}: {r['rows']} rows, {r['text_bytes']} text bytes",
                  f"  format_rows {r['format_ms']} ms {r['format_ms_all']} = {r['format_gbps']} GB/s "
                  f"({100 * r['format_hbm_fraction']:.1f} % of HBM); text to host {r['d2h_ms']} ms ({r['d2h_gbps']} GB/s); "
                  f"np.savetxt {r['savetxt_ms']} ms: {r['format_speedup']}x including the copy",
                  f"  parse_rows {r['parse_ms']} ms {r['parse_ms_all']} = {r['parse_gbps']} GB/s "
                  f"({100 * r['parse_hbm_fraction']:.1f} % of HBM); np.loadtxt {r['loadtxt_ms']} ms: {r['parse_speedup']}x"]
    lines += [f"14-byte unpack, {args.points} points: {u_ms} ms {u_runs} = {unpack['unpack_gbps']} GB/s "
              f"({100 * unpack['unpack_hbm_fraction']:.1f} % of HBM); numpy column_stack {h_ms} ms; "
              f"for scale, uploading 16 B per point takes {up_ms} ms",
              f"  (a warm-cache figure: the {14 * args.points // 1000000} MB payload was uploaded just before the timed runs and is read "
              "again in each of them, so part of it is served from the Infinity Cache, not HBM)",
              "Host figures for the drive's text are estimates: np.savetxt / np.loadtxt were timed once on the first slice",
              f"  ({large['host_rows_timed']} rows: {large['savetxt_ms_all'][0]} ms / {large['loadtxt_ms_all'][0]} ms) and scaled "
              f"by {large['rows']} / {large['host_rows_timed']}; they were not run at that size."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
