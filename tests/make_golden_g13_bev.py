"""Writes tests/golden/g13_bev.npz from the reference's own viewer (tools/vis_inference_bev.py).
Not collected by pytest; needs the reference tree, matplotlib and scipy.  The fixture holds inputs
and the reference's outputs only.

    python tests/make_golden_g13_bev.py --reference REFERENCE_CHECKOUT

The tool creates ./inference_vis_bev and imports matplotlib, scipy and src.* when loaded, so the
maker loads it by file path from a temporary working directory with the checkout on sys.path.
generate_bev_map is the tool's own function.  The tone map (:143-148) is inline in main(): the
maker runs those four numpy calls on the tool's image.  calc_metric (:154-176) and the zoom rule
(:178-214) are nested in main() and cannot be imported: the maker restates them (chamfer_ref,
windows_ref below, in numpy's words, per pair / per item as there) and says so here.

Stored per cloud k: c{k}_pts, c{k}_res, c{k}_pad (inputs); c{k}_image, c{k}_extent, c{k}_p (NaN for
"no positive pixel"), c{k}_norm, c{k}_rgba = matplotlib.colormaps['jet'](norm, bytes=True) with the
pixels the reference masks (image == 0) set to opaque black, its axes background.

Condition asserted so the tests may demand exact colours: for every distinct positive pixel value
below p of a stored image, norm * 256 is at least 1e-4 from an integer (points whose intensity
breaks that are dropped from the cloud before it is stored).  Values >= p are clipped to exactly
1.0, whose power is exactly 1.0, index 255.  No margin is asked of pixel coordinates: the clouds
hold points on and next to pixel edges on purpose."""
import argparse
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g13_bev.npz")


def load_tool(ref_dir):
    os.environ.setdefault("MPLBACKEND", "Agg")
    ref_dir = os.path.abspath(ref_dir)
    sys.path.insert(0, ref_dir)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            spec = importlib.util.spec_from_file_location("ref_vis_bev", os.path.join(ref_dir, "tools", "vis_inference_bev.py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        finally:
            os.chdir(cwd)
    return mod


def tone(image):
    """:143-148 on the tool's image."""
    if image.max() > 0:
        p = np.percentile(image[image > 0], 90)
        norm = np.power(np.clip(image / p, 0, 1), 0.6)
        return norm, p
    return image, None


def chamfer_ref(gt, pred):
    """calc_metric restated: symmetric mean nearest-vertex xy distance, -1.0 without a GT."""
    if gt is None or len(gt) == 0:
        return -1.0
    d = np.linalg.norm(gt[:, None, :2] - pred[None, :, :2], axis=2)
    return (np.mean(d.min(axis=1)) + np.mean(d.min(axis=0))) / 2.0


def windows_ref(items):
    """The zoom rule restated on the scene JSON's items: [(item index, [min_y, max_y, min_x, max_x])]."""
    out = []
    for idx, item in enumerate(items):
        xs, ys = [], []
        gt = item.get("position", [])
        has_gt = len(gt) > 1
        if has_gt:
            xs += [p["x"] for p in gt]; ys += [p["y"] for p in gt]
        cands = item.get("noisy_candidates", [])
        if not cands and not has_gt:
            continue
        for c in cands:
            xs += [p["x"] for p in c]; ys += [p["y"] for p in c]
        if not xs:
            continue
        lo_x, hi_x, lo_y, hi_y = min(xs) - 10.0, max(xs) + 10.0, min(ys) - 10.0, max(ys) + 10.0
        if hi_y - lo_y <= 0 or hi_x - lo_x <= 0:
            continue
        out.append((idx, [lo_y, hi_y, lo_x, hi_x]))
    return out


def near_integer_span(T, res, pad):
    """A span s (a multiple of res) for which T((s + 2 pad)) / T(res) is not an integer but within
    one ulp of one."""
    for k in range(20, 400):
        s = T(k) * T(res)
        q = (s + T(pad) - (T(0) - T(pad))) / T(res)
        r = np.rint(q)
        if q != r and abs(q - r) <= np.spacing(T(r)):
            return s
    raise AssertionError("no span within one ulp of an integer found")


def make_clouds(rng):
    clouds = []
    n = 4000
    u2 = np.column_stack([rng.uniform(0, 6, n), rng.uniform(0, 4, n), rng.uniform(-1, 1, n),
                          rng.integers(0, 65536, n)]).astype(np.float32)
    u2[:40, 3] = 0.0                                               # zero intensities: masked like empty pixels
    clouds.append(("u2_f32", u2, 0.05, 5.0))
    clouds.append(("u2_f64", u2.astype(np.float64), 0.05, 5.0))
    neg = np.column_stack([rng.uniform(0, 3, 1500), rng.uniform(0, 3, 1500), np.zeros(1500),
                           np.round(rng.uniform(-50, 50, 1500), 2)]).astype(np.float32)
    clouds.append(("negative", neg, 0.1, 2.0))
    dense = np.column_stack([rng.uniform(0, 1, 20000), rng.uniform(0, 1, 20000), np.zeros(20000),
                             rng.integers(1, 4000, 20000)]).astype(np.float32)
    clouds.append(("dense", dense, 0.05, 1.0))
    clouds.append(("single", np.array([[3.25, -1.5, 0.2, 77.0]], dtype=np.float32), 0.05, 5.0))
    for T, tag in ((np.float32, "f32"), (np.float64, "f64")):
        s = near_integer_span(T, 0.05, 1.0)
        m = 600
        ulp = np.column_stack([rng.uniform(0, float(s), m), rng.uniform(0, 2, m), np.zeros(m), rng.integers(1, 60000, m)]).astype(T)
        ulp[0, 0], ulp[1, 0] = T(0), s
        clouds.append((f"ulp_{tag}", ulp, 0.05, 1.0))
        # on and next to pixel edges: anchors fix the bounds, then y = y_min + j res and x = x_max - j res
        res, pad = T(0.05), T(1.0)
        anchors = np.array([[0, 0, 0, 5], [4, 3, 0, 6]], dtype=T)
        y_min, x_max = T(0) - pad, T(4) + pad
        rows = []
        for j in range(21, 79):
            for step in (-1, 0, 1):
                y = y_min + T(j) * res
                x = x_max - T(j) * res
                y = np.nextafter(y, T(np.inf) * step) if step else y
                x = np.nextafter(x, T(np.inf) * step) if step else x
                rows.append([T(1.0) + T(j) * res * T(0.5), y, 0, 1000 + 37 * j + step])
                rows.append([x, T(0.5) + T(j) * res * T(0.25), 0, 30000 + 41 * j + step])
        edges = np.concatenate([anchors, np.array(rows, dtype=T)]).astype(T)
        clouds.append((f"edges_{tag}", edges, 0.05, 1.0))
    return clouds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    V = load_tool(args.reference)
    import matplotlib
    jet = matplotlib.colormaps["jet"]
    rng = np.random.default_rng(13)
    out, names = {}, []
    for k, (name, pts, res, pad) in enumerate(make_clouds(rng)):
        for _ in range(50):                                        # drop points that break the colour margin
            image, extent = V.generate_bev_map(pts, res, pad)
            norm, p = tone(image)
            if p is None:
                break
            below = (image > 0) & (image < p)
            nv = norm[below].astype(np.float64) * 256
            offenders = np.unique(image[below][np.abs(nv - np.rint(nv)) < 1e-4])
            if not len(offenders):
                break
            pts = pts[~np.isin(pts[:, 3].astype(np.float32), offenders)]
        else:
            raise AssertionError(f"{name}: the colour margin could not be met")
        assert image.dtype == np.float32 and norm.dtype == np.float32, (image.dtype, norm.dtype)
        assert all(np.asarray(e).dtype == pts.dtype for e in extent), [type(e) for e in extent]
        assert p is None or isinstance(p, np.float32)
        rgba = jet(norm, bytes=True)
        rgba[image == 0] = (0, 0, 0, 255)
        names.append(name)
        out[f"c{k}_pts"], out[f"c{k}_res"], out[f"c{k}_pad"] = pts, np.float64(res), np.float64(pad)
        out[f"c{k}_image"], out[f"c{k}_extent"] = image, np.array(extent, dtype=pts.dtype)
        out[f"c{k}_p"] = np.float32(np.nan if p is None else p)
        out[f"c{k}_norm"], out[f"c{k}_rgba"] = norm, rgba
        print(f"{name}: {len(pts)} points {pts.dtype}, image {image.shape}, {int((image != 0).sum())} lit, p {p}")
    q = (out["c5_extent"][3] - out["c5_extent"][2]) / np.float32(0.05)
    assert q != np.rint(q) and abs(q - np.rint(q)) <= np.spacing(np.float32(np.rint(q)))
    zero = np.zeros((12, 9), dtype=np.float32)
    assert tone(zero)[1] is None
    out["names"] = np.frombuffer(json.dumps(names).encode(), dtype=np.uint8)
    out["jet"] = jet(np.arange(256), bytes=True)
    # calc_metric for a few pairs
    pairs = []
    for m_gt, m_pr in ((32, 32), (5, 32), (32, 3), (1, 7), (17, 1)):
        x = np.sort(rng.uniform(-20, 20, m_gt))
        gt = np.column_stack([x, 0.3 * np.sin(x / 4), rng.normal(0, 0.1, m_gt)])
        xp = np.sort(rng.uniform(-22, 22, m_pr))
        pr = np.column_stack([xp, 0.3 * np.sin(xp / 4) + rng.uniform(-0.5, 0.5), rng.normal(0, 0.1, m_pr)])
        pairs.append((gt, pr))
    out["cm_gt"] = np.concatenate([g for g, _ in pairs]); out["cm_gt_len"] = np.array([len(g) for g, _ in pairs])
    out["cm_pred"] = np.concatenate([p for _, p in pairs]); out["cm_pred_len"] = np.array([len(p) for _, p in pairs])
    out["cm_val"] = np.array([chamfer_ref(g, p) for g, p in pairs])
    assert chamfer_ref(None, pairs[0][1]) == -1.0 and chamfer_ref(np.zeros((0, 3)), pairs[0][1]) == -1.0
    # the windows of a small item list
    dicts = lambda a: [{"x": float(p[0]), "y": float(p[1]), "z": float(p[2])} for p in a]
    line = lambda n, y: np.column_stack([np.sort(rng.uniform(-20, 20, n)), y + rng.normal(0, 0.2, n), np.zeros(n)])
    items = [
        {"position": dicts(line(9, 1.0)), "noisy_candidates": [dicts(line(6, 1.3)), dicts(line(4, 0.6))]},
        {"position": dicts(line(1, 5.0)), "noisy_candidates": []},                       # 1-vertex GT, no candidate: skipped
        {"position": [], "noisy_candidates": [dicts(line(7, -3.0))]},                     # candidates only
        {"position": dicts(line(12, 8.0))},                                               # GT only
        {"noisy_candidates": []},                                                         # nothing: skipped
        {"position": dicts(line(1, 2.0)), "noisy_candidates": [dicts(line(3, 2.5))]},     # 1-vertex GT is not counted
    ]
    wins = windows_ref(items)
    assert [i for i, _ in wins] == [0, 2, 3, 5]
    out["win_items"] = np.frombuffer(json.dumps(items).encode(), dtype=np.uint8)
    out["win_kept"] = np.array([i for i, _ in wins], dtype=np.int64)
    out["win_windows"] = np.array([w for _, w in wins], dtype=np.float64)

    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    assert buf.tell() <= 512 * 1024, buf.tell()
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(f"wrote {OUT} ({buf.tell()} bytes)")


if __name__ == "__main__":
    main()
