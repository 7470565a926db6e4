"""Writes tests/golden/g10_scene_metrics.npz from the reference's own scene-evaluation helpers
(inference_whole_scene.py: crop_gt_to_pred_range, compute_chamfer_distance, calibrate_alignment;
src/dataset.py: resample_polyline).  Not collected by pytest; needs the reference tree and scipy.
The fixture holds inputs and the reference's outputs only.

    python tests/make_golden_g10_scene_metrics.py --reference REFERENCE_CHECKOUT

Row loop and skipping follow the reference's main() (:299-365): a candidate with fewer than 2
vertices is skipped, a row is scored when its item GT has at least 2 vertices, the scene
calibration runs on the raw candidates against every item GT of at least 2 vertices.  Crop
indices are read off the view crop_gt_to_pred_range returns (a slice, reversed or not, of the
GT array).  Every calibration also stores its full coarse and fine tables of per-shift means,
computed with scipy KDTree the way calibrate_alignment does."""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g10_scene_metrics.npz")
M = 32


def load_reference(ref_dir):
    sys.dont_write_bytecode = True
    go = types.ModuleType("plotly.graph_objects")       # plotting only: stubbed
    plotly = types.ModuleType("plotly")
    plotly.graph_objects = go
    sys.modules.setdefault("plotly", plotly)
    sys.modules.setdefault("plotly.graph_objects", go)
    sys.path.insert(0, ref_dir)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:          # the module creates its output directory at import
        os.chdir(tmp)
        try:
            import inference_whole_scene as W
            from src.dataset import resample_polyline
        finally:
            os.chdir(cwd)
    return W, resample_polyline


def P(*pts):
    return np.array(pts, dtype=np.float64).reshape(-1, 3)


def integer_scene():
    """Small integer coordinates: every distance evaluation is exact, so ties are exact ties."""
    items = [
        {"position": P((0, 0, 0), (2, 0, 0), (4, 0, 0), (6, 0, 0)),          # first-index ties at both ends
         "noisy_candidates": [P((1, 0, 0), (5, 0, 0)), P((1, 1, 0), (3, 1, 0), (5, 1, 0))]},
        {"position": P((0, 4, 0), (8, 4, 0)),                                 # exactly 2 vertices
         "noisy_candidates": [P((1, 4, 0), (3, 4, 1), (7, 4, 0))]},
        {"position": P((0, 8, 0), (4, 8, 0), (8, 8, 0), (12, 8, 0)),          # widen at index 0
         "noisy_candidates": [P((-3, 8, 0), (-1, 8, 0))]},
        {"position": P((0, 12, 0), (4, 12, 0), (8, 12, 0), (12, 12, 0)),      # widen at the last index
         "noisy_candidates": [P((13, 12, 0), (15, 12, 0))]},
        {"position": P((12, 16, 0), (8, 16, 0), (4, 16, 0), (0, 16, 0)),      # reversed GT direction
         "noisy_candidates": [P((1, 16, 0), (6, 17, 0), (11, 16, 0))]},
        {"position": P((0, 20, 0), (2, 20, 0), (2, 20, 0), (4, 20, 0), (4, 20, 0), (4, 20, 0), (6, 20, 0)),
         "noisy_candidates": [P((0, 21, 0), (6, 21, 0)), P((2, 19, 0), (4, 19, 0))]},   # duplicate vertices
        {"position": P((0, 24, 0)),                                           # 1-vertex GT: not scored
         "noisy_candidates": [P((0, 24, 0), (2, 24, 0))]},
        {"position": None,                                                    # no position
         "noisy_candidates": [P((0, 28, 0), (4, 28, 0))]},
        {"position": P((0, 32, 0), (4, 32, 0)),                               # a 1-vertex candidate: skipped
         "noisy_candidates": [P((0, 32, 0)), P((0, 32, 1), (4, 32, 1))]},
        {"position": P((0, 40, 0), (10, 40, 0)),                              # bad match (Lat 2 m)
         "noisy_candidates": [P((0, 42, 0), (10, 42, 0))]},
        {"position": P((0, 44, 0), (2, 44, 0)),                               # d_reverse == d_normal: kept
         "noisy_candidates": [P((1, 45, 0), (1, 43, 0))]},
        {"position": P((0, 48, 0), (3, 48, 0), (6, 48, 0)), "noisy_candidates": []},
    ]
    return items


def random_scene(seed, origin, n_lines=8):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n_lines):
        n = int(rng.integers(6, 60))
        x = np.sort(rng.uniform(-30, 30, n))
        if i % 3 == 2:
            x = x[::-1]                                                       # GT runs the other way
        y = 3.5 * i + 0.4 * np.sin(x / 9.0 + i) + rng.normal(0, 0.03, n)
        z = 0.2 * np.cos(x / 17.0) + rng.normal(0, 0.02, n)
        gt = np.stack([x, y, z], 1)
        if i == 5:
            gt = np.insert(gt, 3, gt[3], axis=0)                              # a zero-length segment
        cands = []
        for k in range(int(rng.integers(1, 4))):
            a, b = np.sort(rng.uniform(-35, 35, 2))
            if b - a < 3:
                b = a + 3
            nv = int(rng.integers(2, 40))
            cx = np.linspace(a, b, nv)
            cy = 3.5 * i + 0.4 * np.sin(cx / 9.0 + i) + rng.normal(0, 0.08, nv) + rng.uniform(-0.5, 0.5)
            if k == 2:
                cy = cy + 1.8                                                 # wrong lane: a bad match
            cz = 0.2 * np.cos(cx / 17.0) + rng.normal(0, 0.05, nv)
            c = np.stack([cx, cy, cz], 1)
            if rng.uniform() < 0.4:
                c = c[::-1]
            cands.append(c)
        items.append({"position": gt, "noisy_candidates": cands})
    items.append({"position": None, "noisy_candidates": [items[0]["noisy_candidates"][0] + [0, 0.2, 0]]})
    off = np.asarray(origin, dtype=np.float64)
    for it in items:
        if it["position"] is not None:
            it["position"] = np.ascontiguousarray(it["position"] + off)
        it["noisy_candidates"] = [np.ascontiguousarray(c + off) for c in it["noisy_candidates"]]
    return items


def no_gt_scene():
    return [{"position": None, "noisy_candidates": [P((0, 0, 0), (3, 1, 0), (6, 1, 0))]},
            {"position": P((1, 1, 1)), "noisy_candidates": [P((0, 2, 0), (5, 2, 0))]}]


def crop_indices(gt, crop):
    """(start, end, reversed) of the view crop_gt_to_pred_range returned."""
    assert np.shares_memory(gt, crop)
    first = (crop.__array_interface__["data"][0] - gt.__array_interface__["data"][0]) // gt.strides[0]
    if crop.strides[0] > 0:
        return int(first), int(first + len(crop) - 1), False
    return int(first - len(crop) + 1), int(first), True


def kd_means(KDTree, pred_all, gt_all, shifts):
    tree = KDTree(gt_all)
    return np.array([np.mean(tree.query(pred_all + np.array([dx, dy, 0]))[0]) for dx, dy in shifts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    W, resample_polyline = load_reference(args.reference)
    from scipy.spatial import KDTree

    scenes = [integer_scene(), random_scene(1, (0.0, 0.0, 0.0)), random_scene(2, (4e5, 5e6, 30.0)), no_gt_scene()]
    rng = np.random.default_rng(10)
    d = {k: [] for k in ("item_scene", "item_has_pos", "gt_v", "gt_len", "cand_item", "cand_local", "cand_v",
                         "cand_len", "row_scene", "row_item", "row_item_local", "row_cand_local", "noisy", "refined",
                         "valid", "crop_start", "crop_end", "reversed", "resampled_gt", "ade_noisy", "ade_refined",
                         "cd_noisy", "cd_refined", "lat_noisy", "lat_refined", "bad_match", "cal_done", "cal_dx",
                         "cal_dy", "cal_best", "coarse_means", "fine_len", "fine_shifts", "fine_means")}
    coarse = np.array([(dx, dy) for dx in np.arange(-20, 20, 2.0) for dy in np.arange(-10, 10, 1.0)])
    n_items = 0
    for si, items in enumerate(scenes):
        pred_lines, gt_lines = [], []
        for ii, item in enumerate(items):
            gi = n_items + ii
            gt = item["position"]
            d["item_scene"].append(si)
            d["item_has_pos"].append(gt is not None)
            gt_points = gt if gt is not None else np.empty((0, 3))
            d["gt_v"].append(gt_points)
            d["gt_len"].append(len(gt_points))
            if len(gt_points) > 1:
                gt_lines.append(gt_points)
            for k, c in enumerate(item["noisy_candidates"]):
                d["cand_item"].append(gi)
                d["cand_local"].append(k)
                d["cand_v"].append(c)
                d["cand_len"].append(len(c))
                if len(c) < 2:
                    continue
                pred_lines.append(c)
                noisy = resample_polyline(c, M)
                refined = noisy + rng.normal(0, 0.05, noisy.shape)
                d["row_scene"].append(si); d["row_item"].append(gi)
                d["row_item_local"].append(ii); d["row_cand_local"].append(k)
                d["noisy"].append(noisy); d["refined"].append(refined)
                valid = len(gt_points) > 1
                d["valid"].append(valid)
                if not valid:
                    d["crop_start"].append(-1); d["crop_end"].append(-1); d["reversed"].append(False)
                    d["resampled_gt"].append(np.zeros((M, 3)))
                    for name in ("ade_noisy", "ade_refined", "cd_noisy", "cd_refined", "lat_noisy", "lat_refined"):
                        d[name].append(np.nan)
                    d["bad_match"].append(False)
                    continue
                crop = W.crop_gt_to_pred_range(gt_points, noisy)
                assert len(crop) > 1
                a, b, rev = crop_indices(gt_points, crop)
                d["crop_start"].append(a); d["crop_end"].append(b); d["reversed"].append(rev)
                gt32 = resample_polyline(crop, M)
                d["resampled_gt"].append(gt32)
                d["ade_noisy"].append(np.mean(np.linalg.norm(noisy - gt32, axis=1)))
                d["ade_refined"].append(np.mean(np.linalg.norm(refined - gt32, axis=1)))
                cdn, latn = W.compute_chamfer_distance(noisy, crop)
                cdr, latr = W.compute_chamfer_distance(refined, crop)
                d["cd_noisy"].append(cdn); d["lat_noisy"].append(latn)
                d["cd_refined"].append(cdr); d["lat_refined"].append(latr)
                d["bad_match"].append(bool(latn > 1.0))
        n_items += len(items)
        done = len(pred_lines) > 0 and len(gt_lines) > 0
        d["cal_done"].append(done)
        if not done:
            d["cal_dx"].append(np.nan); d["cal_dy"].append(np.nan); d["cal_best"].append(np.nan)
            d["coarse_means"].append(np.full(len(coarse), np.nan)); d["fine_len"].append(0)
            continue
        (dx, dy), best = W.calibrate_alignment(pred_lines, gt_lines)
        d["cal_dx"].append(dx); d["cal_dy"].append(dy); d["cal_best"].append(best)
        pa, ga = np.vstack(pred_lines), np.vstack(gt_lines)
        cm = kd_means(KDTree, pa, ga, coarse)
        bd, bo = np.inf, (0, 0)
        for (x, y), v in zip(coarse, cm):
            if v < bd:
                bd, bo = v, (x, y)
        fine = np.array([(x, y) for x in np.arange(bo[0] - 2.0, bo[0] + 2.0, 0.2)
                         for y in np.arange(bo[1] - 1.0, bo[1] + 1.0, 0.2)])
        fm = kd_means(KDTree, pa, ga, fine)
        d["coarse_means"].append(cm); d["fine_len"].append(len(fine))
        d["fine_shifts"].append(fine); d["fine_means"].append(fm)
        print(f"scene {si}: {len(pred_lines)} candidates, {len(gt_lines)} GT lines, offset ({dx:.2f}, {dy:.2f}) "
              f"mean {best:.6f}, fine grid {len(fine)}")

    out = {}
    for k, v in d.items():
        if k in ("gt_v", "cand_v", "fine_shifts"):
            out[k] = np.concatenate(v).reshape(-1, 3 if k != "fine_shifts" else 2)
        elif k == "fine_means":
            out[k] = np.concatenate(v)
        else:
            out[k] = np.asarray(v)
    out["coarse_shifts"] = coarse
    out["n_scenes"] = np.int64(len(scenes))
    out["m"] = np.int64(M)
    np.savez_compressed(OUT, **out)
    print(f"rows {len(out['valid'])} (valid {int(out['valid'].sum())}, bad {int(out['bad_match'].sum())}, "
          f"reversed {int(out['reversed'].sum())}); wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
