"""Times the 3-D views (csrc/prh_view.hpp, pointnet_refine_amd/view3d.py).  Each GPU step runs in a
child process of its own under a time limit; a step that fails or times out ends the run.  Device
times are medians of repeats between device events after a warm-up; clocks are not touched.

  splat  prh_view_splat (the launch splat_points makes, timed without the wrapper's camera upload
         and flag read-back; the whole call is reported beside it as wall time) of a generated --points cloud (float32) into one --size x --size view, for a
         close view (the cloud overflows the image: little contention, many points clipped) and a
         zoomed-out view (the whole cloud inside a small part of the image: every point competes for
         few pixels), next to the bytes it must read (points x 16 B) and to bev_map of the same cloud.
  lines  draw_lines3d of a --items item scene (three lines per item) into one overview, and its
         host half (pack_lines3d) on its own.
  scene  render_scene3d of the same scene end to end, with and without PNG files, and its parts
         (refine and metrics / bounds / splat / lines / resolve / PNG encoding).
  host   the numpy restatement of the splat at --host-points points, split over --threads threads
         (a buffer per thread, a final minimum), and on one thread.

    python scripts/view3d_bench.py [--points 20000000] [--size 1000] [--items 256] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bev_render_bench import make_scene, timed  # noqa: E402


def make_cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    pts = np.empty((n, 4), dtype=np.float32)
    pts[:, 0] = rng.uniform(-100, 100, n)
    pts[:, 1] = rng.uniform(-30, 30, n)
    pts[:, 2] = rng.normal(0, 0.3, n)
    pts[:, 3] = rng.integers(0, 60, n)
    return pts


def _host_chunk(pts, cam, h, w, cmin, cmax):
    """The rule's 1 x 1 splat of one chunk in numpy: projection in fp64, then the minimum per pixel by
    a sort and a segmented reduction (both release the interpreter lock).  Returns (pixels, words)."""
    p = pts[:, :3].astype(np.float64)
    q = p - cam[0:3]
    xr = (q[:, 0] * cam[3] + q[:, 1] * cam[4]) + q[:, 2] * cam[5]
    yu = (q[:, 0] * cam[6] + q[:, 1] * cam[7]) + q[:, 2] * cam[8]
    d = (q[:, 0] * cam[9] + q[:, 1] * cam[10]) + q[:, 2] * cam[11]
    ok = d >= cam[13]
    k = cam[12] / d[ok]
    col, row = np.floor(w / 2.0 + xr[ok] * k), np.floor(h / 2.0 - yu[ok] * k)
    inside = (col >= 0) & (col < w) & (row >= 0) & (row < h)
    lut = np.clip(np.floor((pts[ok, 3].astype(np.float64) - cmin) / (cmax - cmin) * 256.0), 0, 255).astype(np.uint64)
    word = (d[ok].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(0x01000000) | lut
    pix, word = (row[inside] * w + col[inside]).astype(np.int64), word[inside]
    if len(pix) == 0:
        return pix, word
    order = np.argsort(pix, kind="stable")
    pix, word = pix[order], word[order]
    first = np.flatnonzero(np.concatenate(([True], pix[1:] != pix[:-1])))
    return pix[first], np.minimum.reduceat(word, first)


def host_splat(pts, cam, h, w, cmin, cmax, threads):
    """The cloud in `threads` chunks on a thread pool, a buffer per chunk, a final minimum over the buffers."""
    from concurrent.futures import ThreadPoolExecutor
    chunks = np.array_split(np.arange(len(pts)), max(threads, 1))
    with ThreadPoolExecutor(max(threads, 1)) as pool:
        parts = list(pool.map(lambda c: _host_chunk(pts[c[0]:c[-1] + 1], cam, h, w, cmin, cmax) if len(c) else None, chunks))
    z = np.full(h * w, np.uint64(0xFFFFFFFFFFFFFFFF))
    for part in parts:
        if part is not None and len(part[0]):
            z[part[0]] = np.minimum(z[part[0]], part[1])
    return z.reshape(h, w)


def step_splat(args):
    import torch
    from pointnet_refine_amd import bev as B
    from pointnet_refine_amd import view3d as V
    pts = make_cloud(args.points)
    dev = torch.from_numpy(pts).cuda()
    s = args.size
    lo, hi = V.view_bounds(dev)
    bounds_ms, _ = timed(lambda: V.view_bounds(dev), args.reps)
    out = {"step": "splat", "device": torch.cuda.get_device_name(0), "points": args.points, "image": [s, s],
           "read_GB": round(args.points * 16 / 1e9, 3), "view_bounds_ms": round(bounds_ms, 3)}
    fit = V.fit_camera((lo, hi), 35.0, 180.0, height=s, width=s)
    cams = {"close": V.orbit_camera((0.0, 0.0, 0.0), 35.0, 180.0, 25.0, height=s, width=s),
            "fit": fit,
            "far": V.orbit_camera((0.0, 0.0, 0.0), 35.0, 180.0, 8.0 * float(np.linalg.norm(fit[0:3])), height=s, width=s)}
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    bad = torch.zeros((1,), dtype=torch.int32, device=dev.device)

    def launch(z, cam_t, n_views, size):
        """prh_view_splat alone: no camera upload, no read-back of the flag."""
        L.check(L.lib().prh_view_splat(G.ptr(dev), dev.shape[0], 0, G.ptr(cam_t), n_views, None, 0, None, size, 1.0, 40.0, s, s,
                                       G.ptr(z), G.ptr(bad), dev.device.index, G.stream(dev.device)), "prh_view_splat")

    def fresh_ms(z, cam_t, n_views, size):
        """The launch on a just-cleared buffer (the clear is outside the events): no plain-load skips at the start."""
        out = []
        for _ in range(args.reps):
            z.fill_(-1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(z, cam_t, n_views, size)
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return float(np.median(out)), [round(v, 3) for v in out]

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, cam in cams.items():
        cam_t = torch.from_numpy(cam[None].copy()).cuda()
        for size in (1, 2):
            z = V.new_zbuffer(1, s, s)
            V.splat_points(z, dev, cam[None], size, 1.0, 40.0)
            lit = int((z != -1).sum().item())
            ms, all_ms = timed(lambda: launch(z, cam_t, 1, size), args.reps)
            fms, fresh = fresh_ms(z, cam_t, 1, size)
            call_ms = float(np.median([wall(lambda: V.splat_points(z, dev, cam[None], size, 1.0, 40.0)) for _ in range(5)]))
            out[f"{name}_k{size}"] = {"lit_pixels": lit, "filled_buffer_kernel_ms": round(ms, 3), "filled_buffer_kernel_ms_all": all_ms,
                                      "fresh_buffer_kernel_ms": round(fms, 3), "fresh_buffer_kernel_ms_all": fresh,
                                      "fresh_read_GB_per_s": round(args.points * 16 / 1e9 / (fms * 1e-3), 1),
                                      "splat_points_call_wall_ms": round(call_ms, 3)}
    three = np.stack([cams["close"], cams["fit"], cams["far"]])
    three_t = torch.from_numpy(three.copy()).cuda()
    ms3, _ = fresh_ms(V.new_zbuffer(3, s, s), three_t, 3, 1)
    out["three_views_k1_fresh_kernel_ms"] = round(ms3, 3)
    bev_ms, _ = timed(lambda: B.bev_map(dev), args.reps)
    out["bev_map_ms"] = round(bev_ms, 3)
    z = V.new_zbuffer(1, s, s)
    res_ms, _ = timed(lambda: V.resolve(z, V.jet_table()), args.reps)
    out["resolve_ms"] = round(res_ms, 3)
    return out


def scene_lines(items):
    lines, styles = [], []
    from pointnet_refine_amd import view3d as V
    for it in items:
        lines += [it["position"], it["noisy_candidates"][0], it["noisy_candidates"][0] + np.array([0.0, 0.1, 0.0])]
        styles += [V.STYLE_GT, V.STYLE_NOISY, V.STYLE_REFINED]
    return lines, styles


def step_lines(args):
    import torch
    from pointnet_refine_amd import view3d as V
    items, cloud = make_scene(args.items)
    lines, styles = scene_lines(items)
    s = args.size
    cam = V.fit_camera(cloud, 35.0, 180.0, height=s, width=s, target=(0.0, 0.0, 0.0))[None]
    z = V.new_zbuffer(1, s, s)
    t = time.perf_counter()
    for _ in range(3):
        segs, ids, st = V.pack_lines3d(lines, styles, cam, s, s)
    pack_ms = (time.perf_counter() - t) * 1e3 / 3
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    segs_t, ids_t, st_t, cam_t = up(segs), up(ids), up(st), up(cam)
    dev = z.device
    kernel = lambda: L.check(L.lib().prh_view_lines(G.ptr(segs_t), G.ptr(ids_t), len(segs), G.ptr(st_t), len(st), G.ptr(cam_t),
                                                    1, s, s, G.ptr(z), dev.index, G.stream(dev)), "prh_view_lines")
    k_ms, k_all = timed(kernel, args.reps)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    call_ms = float(np.median([wall(lambda: V.draw_lines3d(z, lines, styles, cam)) for _ in range(5)]))
    ex, ey = segs[:, 2] - segs[:, 0], segs[:, 3] - segs[:, 1]
    box = (np.abs(ex) + 4) * (np.abs(ey) + 4)
    return {"step": "lines", "items": len(items), "lines": len(lines), "segments": int(len(segs)), "image": [s, s],
            "pack_lines3d_host_ms": round(pack_ms, 2), "view_lines_kernel_ms": round(k_ms, 3), "view_lines_kernel_ms_all": k_all,
            "draw_lines3d_call_ms": round(call_ms, 2), "mean_box_pixels": round(float(box.mean()), 1),
            "max_box_pixels": round(float(box.max()), 1)}


def step_scene(args):
    import torch
    from pointnet_refine_amd import bev as B
    from pointnet_refine_amd import view3d as V
    from pointnet_refine_amd.metrics import evaluate_scene
    from pointnet_refine_amd.model import LineRefineNet
    items, cloud = make_scene(args.items)
    torch.manual_seed(0)
    model = LineRefineNet().cuda().eval()

    def wall(fn):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    med = lambda fn, k=5: float(np.median([wall(fn) for _ in range(k)]))
    with tempfile.TemporaryDirectory() as tmp:
        V.render_scene3d(model, cloud, items, out_dir=tmp, name="w")        # warm-up
        end_ms = med(lambda: V.render_scene3d(model, cloud, items))
        close_ms = med(lambda: V.render_scene3d(model, cloud, items, closeups=True), 3)
        file_ms = med(lambda: V.render_scene3d(model, cloud, items, out_dir=tmp, name="s"), 3)
        res = V.render_scene3d(model, cloud, items)
        dev = torch.from_numpy(cloud).cuda()
        eval_ms = med(lambda: evaluate_scene(model, dev, items))
        bounds_ms = med(lambda: V.view_bounds(dev))
        cams, lines, styles = res["cameras"], res["lines"], res["styles"]
        h, w = res["rgba"].shape[1:3]
        splat_ms = med(lambda: V.splat_points(V.new_zbuffer(len(cams), h, w), dev, cams, 2, 1.0, 40.0))
        z = V.splat_points(V.new_zbuffer(len(cams), h, w), dev, cams, 2, 1.0, 40.0)
        lines_ms = med(lambda: V.draw_lines3d(z, lines, styles, cams))
        resolve_ms = med(lambda: V.resolve(z, V.jet_table(), styles))
        host = res["rgba"].cpu().numpy()
        t = time.perf_counter()
        for k, v in enumerate(host):
            B.write_png(os.path.join(tmp, f"p{k}.png"), v)
        png_ms = (time.perf_counter() - t) * 1e3
    return {"step": "scene", "items": len(items), "cloud_points": len(cloud), "lines": len(lines), "image": [int(h), int(w)],
            "render_scene3d_ms": round(end_ms, 2), "render_scene3d_closeups_ms": round(close_ms, 2),
            "render_scene3d_with_png_ms": round(file_ms, 2), "evaluate_scene_ms": round(eval_ms, 2),
            "view_bounds_ms": round(bounds_ms, 3), "splat_ms": round(splat_ms, 3), "lines_ms": round(lines_ms, 3),
            "resolve_ms": round(resolve_ms, 3), "png_encode_ms": round(png_ms, 1)}


def step_host(args):
    n, s = args.host_points, args.size
    pts = make_cloud(n)
    from pointnet_refine_amd import view3d as V
    lo, hi = pts[:, :3].min(0).astype(np.float64), pts[:, :3].max(0).astype(np.float64)
    cam = V.fit_camera((lo, hi), 35.0, 180.0, height=s, width=s)
    host_splat(pts[:1000], cam, s, s, 1.0, 40.0, args.threads)
    t = time.perf_counter()
    z = host_splat(pts, cam, s, s, 1.0, 40.0, args.threads)
    ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    host_splat(pts, cam, s, s, 1.0, 40.0, 1)
    ms1 = (time.perf_counter() - t) * 1e3
    out = {"step": "host", "host_points": n, "image": [s, s], "host_threads": args.threads, "host_splat_ms": round(ms, 1),
           "host_ns_per_point": round(ms * 1e6 / n, 1), "host_splat_one_thread_ms": round(ms1, 1)}
    import torch
    if torch.cuda.is_available():
        zg = V.splat_points(V.new_zbuffer(1, s, s), pts, cam[None], 1, 1.0, 40.0)
        out["equal_to_device"] = bool(np.array_equal(zg.cpu().numpy().view(np.uint64)[0], z))
    return out


STEPS = {"splat": step_splat, "lines": step_lines, "scene": step_scene, "host": step_host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--host-points", type=int, default=2_000_000)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=300, help="seconds per step")
    ap.add_argument("--steps", default="splat,lines,scene,host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(STEPS[args.step](args)))
        return
    lines = []
    env = dict(os.environ, OMP_NUM_THREADS=str(args.threads))
    for step in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [a for a in sys.argv[1:]]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit, env=env)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step} ran past {args.limit} s; stopping")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"step {step} ended with status {r.returncode}; stopping")
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
