"""Scene-evaluation kernels (csrc/prh_metrics.hpp, pointnet_refine_amd/metrics.py) against the
reference's outputs in the g10 fixture and against the numpy restatement in test_metrics_cpu.py."""
import numpy as np
import pytest
import torch

import test_metrics_cpu as R

pytestmark = pytest.mark.gpu

ABS, REL = 1e-8, 1e-12


def _flat_rows(z):
    return z["noisy"], z["refined"], z["gts"], z["row_item"]


def test_line_metrics_matches_reference(golden_dir):
    from pointnet_refine_amd.metrics import line_metrics
    z = R.load_g10(golden_dir)
    noisy, refined, gts, idx = _flat_rows(z)
    got = line_metrics(noisy, refined, gts, idx)
    for k in ("crop_start", "crop_end", "reversed", "valid", "bad_match"):
        assert np.array_equal(got[k], z[k]), (k, np.flatnonzero(got[k] != z[k]))
    assert R.close(got["resampled_gt"], z["resampled_gt"], ABS, REL)
    for k in R.M_KEYS:
        bad = ~((np.isnan(got[k]) & np.isnan(z[k])) | (np.abs(got[k] - z[k]) <= ABS + REL * np.abs(z[k])))
        assert not bad.any(), (k, np.flatnonzero(bad), got[k][bad], z[k][bad])
    # the same call on CUDA tensors, twice: bitwise equal
    again = line_metrics(torch.from_numpy(noisy).cuda(), torch.from_numpy(refined).cuda(), gts, idx)
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=got[k].dtype.kind == "f"), k


def test_line_metrics_long_gt_and_large_m():
    """Thousands of GT vertices (several LDS chunks), zero-length segments, M = 128 and M = 2."""
    from pointnet_refine_amd.metrics import line_metrics
    rng = np.random.default_rng(3)
    gts, noisy, refined = [], {128: [], 2: []}, {128: [], 2: []}
    for i in range(6):
        n = [2, 3, 130, 700, 2500, 4099][i]
        x = np.cumsum(rng.uniform(0.0, 0.5, n)) + 3e5
        g = np.stack([x, 4e6 + 2.0 * np.sin(x / 40.0), rng.normal(20, 0.1, n)], 1)
        g[n // 2] = g[n // 2 - 1]                                    # a zero-length segment
        if i % 2:
            g = g[::-1].copy()
        gts.append(g)
        a, b = np.sort(rng.uniform(x.min(), x.max(), 2))
        for m in (128, 2):
            c = np.stack([np.linspace(a, b, 7), 4e6 + 2.0 * np.sin(np.linspace(a, b, 7) / 40.0) + 0.3,
                          np.full(7, 20.0)], 1)
            nz = R.resample_ref(c, m)
            noisy[m].append(nz)
            refined[m].append(nz + rng.normal(0, 0.1, nz.shape))
    for m in (128, 2):
        got = line_metrics(np.stack(noisy[m]), np.stack(refined[m]), gts)
        for r in range(len(gts)):
            want = R.line_metrics_ref(noisy[m][r], refined[m][r], gts[r])
            assert (got["crop_start"][r], got["crop_end"][r], got["reversed"][r]) == \
                (want["crop_start"], want["crop_end"], want["reversed"])
            assert R.close(got["resampled_gt"][r], want["resampled_gt"], ABS, REL), (m, r)
            for k in R.M_KEYS:
                assert R.close(got[k][r], want[k], ABS, REL), (m, r, k)


def test_calibrate_alignment_matches_reference(golden_dir):
    from pointnet_refine_amd.metrics import calibrate_alignment
    z = R.load_g10(golden_dir)
    for s in range(int(z["n_scenes"])):
        _, pred, gt = R.g10_scene(z, s)
        if not z["cal_done"][s]:
            continue
        (dx, dy), best, tables = calibrate_alignment(pred, gt, return_tables=True)
        assert abs(best - z["cal_best"][s]) <= 1e-10 * z["cal_best"][s], (s, best, z["cal_best"][s])
        assert R.close(tables["coarse"][1], z["coarse_means"][s], 0.0, 1e-10)
        ref_off = (z["cal_dx"][s], z["cal_dy"][s])
        shifts = np.concatenate([z["coarse_shifts"], z["fine"][s][0]])
        means = np.concatenate([z["coarse_means"][s], z["fine"][s][1]])
        others = means[~((shifts[:, 0] == ref_off[0]) & (shifts[:, 1] == ref_off[1]))]
        margin = (others.min() - z["cal_best"][s]) / z["cal_best"][s]
        if margin > 1e-9:
            assert (dx, dy) == ref_off, (s, (dx, dy), ref_off)
        else:                               # a near-tie: the chosen shift must be as good as the best
            mine = means[(shifts[:, 0] == dx) & (shifts[:, 1] == dy)]
            assert len(mine) and mine.min() - z["cal_best"][s] <= 1e-9, (s, (dx, dy), ref_off)
    assert calibrate_alignment([], gt) == ((0, 0), 999.0)


@pytest.mark.parametrize("P,G,S", [(1000, 777, 37), (300, 1, 5), (257, 1300, 1), (130, 515, 600)])
def test_shift_sweep_matches_restatement(P, G, S):
    from pointnet_refine_amd.metrics import shift_sweep
    rng = np.random.default_rng(P + G + S)
    origin = np.array([4e5, 5e6, 30.0])
    pred = rng.uniform(-30, 30, (P, 3)) * [1, 1, 0.05] + origin
    gt = rng.uniform(-30, 30, (G, 3)) * [1, 1, 0.05] + origin
    shifts = rng.uniform(-20, 20, (S, 2)).round(1)
    got = shift_sweep(pred, gt, shifts)
    want = R.sweep_ref(pred, gt, shifts)
    assert got.shape == (S,)
    assert R.close(got, want, 0.0, 1e-12), np.abs(got / want - 1).max()
    again = shift_sweep(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), shifts)
    assert np.array_equal(got, again)


def _synthetic_scene(seed=5):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(6):
        n = int(rng.integers(4, 30))
        x = np.sort(rng.uniform(-20, 20, n))
        gt = np.stack([x, 3.5 * i + 0.2 * np.sin(x / 5.0), np.zeros(n)], 1)
        cands = []
        for k in range(3):
            nv = [1, 5, 12][(i + k) % 3]
            cx = np.linspace(rng.uniform(-20, -5), rng.uniform(5, 20), nv)
            cands.append(np.stack([cx, 3.5 * i + 0.2 * np.sin(cx / 5.0) + rng.uniform(-0.4, 0.4),
                                   rng.normal(0, 0.02, nv)], 1))
        items.append({"position": gt if i != 2 else None, "noisy_candidates": cands, "context_lines": []})
    items[4]["position"] = items[4]["position"][:1]                   # a 1-vertex GT
    xyz = np.stack([rng.uniform(-22, 22, 30000), rng.uniform(-2, 20, 30000), rng.normal(0, 0.05, 30000)], 1)
    cloud = np.column_stack([xyz, rng.uniform(0, 60, 30000)]).astype(np.float32)
    return items, cloud


def test_evaluate_scene_synthetic():
    from oracle import procedural as P
    from pointnet_refine_amd.io import refine_scene
    from pointnet_refine_amd.metrics import calibrate_alignment, evaluate_scene
    from pointnet_refine_amd.model import LineRefineNet
    items, cloud = _synthetic_scene()
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0))
    m = m.cuda()
    res = evaluate_scene(m, cloud, items, num_context_points=256, crop_radius=0.5, batch_lines=7, seed=3)
    # rows and skipping as the reference's loop (:299-337)
    rows = [(i, k) for i, it in enumerate(items) for k, c in enumerate(it["noisy_candidates"]) if len(c) >= 2]
    assert list(zip(res["item_index"], res["candidate_index"])) == rows
    raw = [items[i]["noisy_candidates"][k] for i, k in rows]
    # refined lines: refine_scene's path, to fp32 rounding
    ref_refined, _ = refine_scene(m, cloud, raw, num_context_points=256, crop_radius=0.5, batch_lines=7, seed=3)
    assert np.abs(res["refined"] - ref_refined).max() < 1e-4
    for r, line in enumerate(raw):
        assert R.close(res["noisy"][r], R.resample_ref(line, 32), 1e-9, 1e-12)
    # metrics: the restatement applied to its own outputs
    for r, (i, k) in enumerate(rows):
        gt = items[i]["position"]
        want = R.line_metrics_ref(res["noisy"][r], res["refined"][r], gt)
        assert res["valid"][r] == want["valid"] == (gt is not None and len(gt) >= 2)
        assert res["bad_match"][r] == want["bad_match"]
        for key in R.M_KEYS:
            assert R.close(res[key][r], want[key], ABS, REL), (r, key)
    cal_gt = [it["position"] for it in items if it["position"] is not None and len(it["position"]) > 1]
    assert res["calibration"] == calibrate_alignment(raw, cal_gt)
    best, off = R.pick(R.coarse_grid(), R.sweep_ref(np.vstack(raw), np.vstack(cal_gt), R.coarse_grid()))
    best, off = R.pick(R.fine_grid(*off), R.sweep_ref(np.vstack(raw), np.vstack(cal_gt), R.fine_grid(*off)), best, off)
    assert abs(res["calibration"][1] - best) <= 1e-10 * best
    assert res["calibration_refined"] == calibrate_alignment(list(res["refined"]), cal_gt)
    # a scene without GT: rows but no calibration
    no_gt = [{"position": None, "noisy_candidates": items[0]["noisy_candidates"], "context_lines": []}]
    res2 = evaluate_scene(m, cloud, no_gt, num_context_points=256, crop_radius=0.5)
    assert res2["calibration"] is None and not res2["valid"].any() and len(res2["valid"]) == 2
