"""Times BEV rendering (csrc/prh_bev.hpp, pointnet_refine_amd/bev.py).  Each GPU step runs in a
child process of its own under a time limit; a step that fails or times out ends the run.  Device
times are medians of repeats between device events after a warm-up; clocks are not touched.

  map    bev_map of a generated --points cloud (float32, integer intensities) and bev_maps of the
         --slices slices drive.slice_cloud cuts from it, against a numpy restatement of the
         reference's generate_bev_map (argsort by intensity, last write wins - the image the
         fixture-checked maximum-per-pixel gives) on the host.  Reports the bytes bev_map must read
         (points x 16 B) over its time.
  scene  render_scene of a --items item scene end to end, with and without PNG files, and its
         parts (refine / image / overlays / PNG encoding); where matplotlib imports, a figure per
         item in the reference's manner (imshow of the whole image, zoom, three plots, savefig) for
         --mpl-items items, reported per item.

    python scripts/bev_render_bench.py [--points 20000000] [--slices 80] [--items 256] [--out FILE]
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


def host_bev_map(pts, res=0.05, pad=5.0):
    """The reference's method in numpy: bounds, indices, argsort by intensity, scatter."""
    x, y, inten = pts[:, 0], pts[:, 1], pts[:, 3]
    x_min, x_max, y_min, y_max = x.min() - pad, x.max() + pad, y.min() - pad, y.max() + pad
    w, h = int((y_max - y_min) / res), int((x_max - x_min) / res)
    img = np.zeros((h, w), dtype=np.float32)
    u, v = ((y - y_min) / res).astype(np.int32), ((x_max - x) / res).astype(np.int32)
    ok = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    u, v, inten = u[ok], v[ok], inten[ok]
    order = np.argsort(inten)
    img[v[order], u[order]] = inten[order]
    return img


def timed(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), [round(v, 3) for v in out]


def step_map(args):
    import torch
    from pointnet_refine_amd import bev as B
    from pointnet_refine_amd import drive as D
    rng = np.random.default_rng(0)
    n = args.points
    length = 25.0 * (args.slices + 1)
    pts = np.empty((n, 4), dtype=np.float32)
    pts[:, 0] = rng.uniform(0, length, n)
    pts[:, 1] = rng.uniform(-30, 30, n)
    pts[:, 2] = rng.normal(0, 0.3, n)
    pts[:, 3] = rng.integers(0, 65536, n)
    dev = torch.from_numpy(pts).cuda()
    img, _ = B.bev_map(dev)
    ms, all_ms = timed(lambda: B.bev_map(dev), args.reps)
    poses = np.zeros((args.slices, 7))
    poses[:, 0] = 25.0 * (np.arange(args.slices) + 1)
    poses[:, 6] = 1.0
    spts, soff, _ = D.slice_cloud(dev, poses)
    extent = (-35.0, 35.0, -27.0, 27.0)
    maps = B.bev_maps(spts, soff, extent)
    ms_s, all_s = timed(lambda: B.bev_maps(spts, soff, extent), args.reps)
    t = time.perf_counter()
    want = host_bev_map(pts)
    host_ms = (time.perf_counter() - t) * 1e3
    equal = bool(np.array_equal(img.cpu().numpy(), want))
    sp, so = spts.cpu().numpy(), soff.cpu().numpy()
    t = time.perf_counter()
    for s in range(args.slices):                                  # the reference renders slice by slice
        if so[s + 1] > so[s]:
            host_bev_map(sp[so[s]:so[s + 1]])
    host_s_ms = (time.perf_counter() - t) * 1e3
    gb = n * 16 / 1e9
    return {"step": "map", "device": torch.cuda.get_device_name(0), "points": n, "image": list(img.shape),
            "lit_pixels": int((img != 0).sum().item()), "bev_map_ms": round(ms, 3), "bev_map_ms_all": all_ms,
            "read_GB": round(gb, 3), "read_GB_per_s": round(gb / (ms * 1e-3), 1),
            "slices": args.slices, "slice_points": int(so[-1]), "slice_maps": list(maps.shape),
            "bev_maps_ms": round(ms_s, 3), "bev_maps_ms_all": all_s,
            "slice_read_GB_per_s": round(int(so[-1]) * 32 / 1e9 / (ms_s * 1e-3), 1),
            "host_bev_map_ms": round(host_ms, 1), "host_bev_maps_ms": round(host_s_ms, 1), "host_threads": args.threads,
            "equal_to_host": equal, "speedup_map": round(host_ms / ms, 1), "speedup_maps": round(host_s_ms / ms_s, 1)}


def make_scene(n_items, seed=1):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n_items):
        x = np.sort(rng.uniform(-24, 24, 30))
        lane = 3.5 * (i % 12) - 20 + 0.3 * np.sin(x / 6.0)
        gt = np.column_stack([x, lane, np.zeros(30)])
        cx = np.linspace(-22, 22, 20)
        cand = np.column_stack([cx, 3.5 * (i % 12) - 20 + 0.3 * np.sin(cx / 6.0) + rng.uniform(-0.4, 0.4), np.zeros(20)])
        items.append({"position": gt, "noisy_candidates": [cand], "context_lines": []})
    n = 400_000
    cloud = np.column_stack([rng.uniform(-25, 25, n), rng.uniform(-25, 25, n), rng.normal(0, 0.05, n),
                             rng.integers(1, 4000, n)]).astype(np.float32)
    return items, cloud


def step_scene(args):
    import torch
    from pointnet_refine_amd import bev as B
    from pointnet_refine_amd.io import refine_scene
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
        B.render_scene(model, cloud, items, out_dir=tmp, name="w")          # warm-up
        end_ms = med(lambda: B.render_scene(model, cloud, items))
        file_ms = med(lambda: B.render_scene(model, cloud, items, out_dir=tmp, name="s"), 3)
        res = B.render_scene(model, cloud, items)
        cands = [it["noisy_candidates"][0] for it in items]
        refine_ms = med(lambda: refine_scene(model, cloud, cands, 32, 2048, 0.5))
        dev = torch.from_numpy(cloud).cuda()

        def image():
            img, ext = B.bev_map(dev)
            norm, _ = B.tone_map(img)
            return B.colorize(norm, img), ext
        image_ms = med(image)
        rgba, ext = image()
        windows, kept = B.item_windows(items)
        crop_ms = med(lambda: B.crop_views(rgba, ext, windows))
        views = B.crop_views(rgba, ext, windows)
        lines, lv, st = [], [], []
        for k in range(len(kept)):
            lines += [items[k]["position"], cands[k], res["refined"][k]]
            lv += [k, k, k]; st += [B.STYLE_GT, B.STYLE_NOISY, B.STYLE_REFINED]
        draw_ms = med(lambda: B.draw_lines(views, None, lines, lv, st))
        host = [res["views"][k].cpu().numpy() for k in range(len(kept))]
        t = time.perf_counter()
        for k, v in enumerate(host):
            B.write_png(os.path.join(tmp, f"p{k}.png"), v)
        png_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        host_bev_map(cloud)
        host_image_ms = (time.perf_counter() - t) * 1e3
        mpl_ms = None
        try:
            os.environ.setdefault("MPLBACKEND", "Agg")
            import matplotlib.pyplot as plt
            img = res["image"].cpu().numpy()
            shown = np.ma.masked_where(img == 0, np.power(np.clip(img / res["p"], 0, 1), 0.6))
            t = time.perf_counter()
            for k in range(min(args.mpl_items, len(kept))):
                w = windows[k]
                fig, ax = plt.subplots(figsize=(8, 8 * min(max((w[3] - w[2]) / (w[1] - w[0]), 0.2), 5)), dpi=100)
                ax.set_facecolor("black")
                ax.imshow(shown, cmap="jet", extent=[float(e) for e in res["extent"]], origin="upper", interpolation="nearest")
                ax.set_xlim(w[0], w[1]); ax.set_ylim(w[2], w[3])
                for line, kw in ((lines[3 * k], dict(color="lime", linewidth=2.0, alpha=0.8)),
                                 (lines[3 * k + 1], dict(color="red", linewidth=1.5, linestyle="--")),
                                 (lines[3 * k + 2], dict(color="cyan", linewidth=2.0, alpha=0.9))):
                    ax.plot(line[:, 1], line[:, 0], **kw)
                fig.tight_layout()
                fig.savefig(os.path.join(tmp, f"m{k}.png"))
                plt.close(fig)
            mpl_ms = (time.perf_counter() - t) * 1e3 / max(min(args.mpl_items, len(kept)), 1)
        except ImportError:
            pass
    pixels = int(res["views"].offsets[-1])
    return {"step": "scene", "device": torch.cuda.get_device_name(0), "items": len(kept), "cloud_points": len(cloud),
            "view_pixels": pixels, "render_scene_ms": round(end_ms, 2), "render_scene_with_png_ms": round(file_ms, 2),
            "refine_ms": round(refine_ms, 2), "image_ms": round(image_ms, 3), "crop_ms": round(crop_ms, 3),
            "overlays_ms": round(draw_ms, 3), "png_encode_ms": round(png_ms, 1),
            "host_image_ms": round(host_image_ms, 1),
            "matplotlib_ms_per_item": None if mpl_ms is None else round(mpl_ms, 1),
            "matplotlib_items_timed": min(args.mpl_items, len(kept)) if mpl_ms is not None else 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--slices", type=int, default=80)
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--mpl-items", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=400, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"map": step_map, "scene": step_scene}[args.step](args)))
        return
    lines = []
    for step in ("map", "scene"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [a for a in sys.argv[1:]]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
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
