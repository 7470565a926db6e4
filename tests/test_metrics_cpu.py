"""Scene-evaluation metrics, host side: a numpy brute-force restatement of the reference's
helpers (inference_whole_scene.py:26-92,148-193; src/dataset.py:8-29) pinned against the g10
fixture the reference produced, and the GPU-only functions refusing to run without a GPU.
Brute force is exact nearest-neighbour search, as scipy's KDTree is.  The GPU tests
(test_metrics_gpu.py) hold the HIP kernels to this restatement."""
import os

import numpy as np
import pytest
import torch

M_KEYS = ("ade_noisy", "ade_refined", "cd_noisy", "cd_refined", "lat_noisy", "lat_refined")


def norm_rows(a):
    a = np.asarray(a, dtype=np.float64)
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def resample_ref(points, m):
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(points) < 2:
        return np.zeros((m, 3))
    cum = np.concatenate(([0.0], np.cumsum(norm_rows(points[1:] - points[:-1]))))
    t = np.linspace(0, cum[-1], m)
    return np.stack([np.interp(t, cum, points[:, k]) for k in range(3)], axis=1)


def crop_ref(gt, noisy):
    """(start, end, reversed) of crop_gt_to_pred_range(gt, noisy); gt has >= 2 vertices."""
    ps, pe = noisy[0], noisy[-1]
    i_s, i_e = int(np.argmin(norm_rows(gt - ps))), int(np.argmin(norm_rows(gt - pe)))
    a, b = min(i_s, i_e), max(i_s, i_e)
    if a == b:
        a, b = max(0, a - 1), min(len(gt) - 1, b + 1)
    d_normal = norm_rows(gt[a] - ps) + norm_rows(gt[b] - pe)
    d_reverse = norm_rows(gt[a] - pe) + norm_rows(gt[b] - ps)
    return a, b, bool(d_reverse < d_normal)


def nn_dist(q, r, chunk=4096):
    """Distance from every row of q to its nearest row of r (brute force)."""
    out = np.empty(len(q))
    for s in range(0, len(q), chunk):
        d = norm_rows(q[s:s + chunk, None, :] - r[None, :, :])
        out[s:s + chunk] = d.min(axis=1)
    return out


def chamfer_ref(pred, gt):
    p2g = np.mean(nn_dist(pred, gt))
    return p2g + np.mean(nn_dist(gt, pred)), p2g


def line_metrics_ref(noisy, refined, gt):
    m = len(noisy)
    if gt is None or len(gt) < 2:
        return dict(valid=False, crop_start=-1, crop_end=-1, reversed=False, resampled_gt=np.zeros((m, 3)),
                    **{k: np.nan for k in M_KEYS}, bad_match=False)
    a, b, rev = crop_ref(gt, noisy)
    crop = gt[a:b + 1][::-1] if rev else gt[a:b + 1]
    g32 = resample_ref(crop, m)
    cdn, latn = chamfer_ref(noisy, crop)
    cdr, latr = chamfer_ref(refined, crop)
    return dict(valid=True, crop_start=a, crop_end=b, reversed=rev, resampled_gt=g32,
                ade_noisy=np.mean(norm_rows(noisy - g32)), ade_refined=np.mean(norm_rows(refined - g32)),
                cd_noisy=cdn, cd_refined=cdr, lat_noisy=latn, lat_refined=latr, bad_match=bool(latn > 1.0))


def sweep_ref(pred, gt, shifts):
    pred, gt = np.asarray(pred, np.float64).reshape(-1, 3), np.asarray(gt, np.float64).reshape(-1, 3)
    return np.array([np.mean(nn_dist(pred + np.array([dx, dy, 0]), gt)) for dx, dy in np.asarray(shifts).reshape(-1, 2)])


def coarse_grid():
    return np.array([(dx, dy) for dx in np.arange(-20, 20, 2.0) for dy in np.arange(-10, 10, 1.0)])


def fine_grid(bx, by):
    return np.array([(dx, dy) for dx in np.arange(bx - 2.0, bx + 2.0, 0.2) for dy in np.arange(by - 1.0, by + 1.0, 0.2)])


def pick(shifts, means, best=np.inf, off=(0, 0)):
    for (dx, dy), v in zip(shifts, means):
        if v < best:
            best, off = v, (dx, dy)
    return best, off


# ------------------------------------------------------------------ the g10 fixture, unpacked
def load_g10(golden_dir):
    z = dict(np.load(os.path.join(golden_dir, "g10_scene_metrics.npz")))
    goff = np.concatenate([[0], np.cumsum(z["gt_len"])])
    coff = np.concatenate([[0], np.cumsum(z["cand_len"])])
    foff = np.concatenate([[0], np.cumsum(z["fine_len"])])
    z["gts"] = [z["gt_v"][goff[i]:goff[i + 1]] if z["item_has_pos"][i] else None for i in range(len(z["gt_len"]))]
    z["cands"] = [z["cand_v"][coff[i]:coff[i + 1]] for i in range(len(z["cand_len"]))]
    z["fine"] = [(z["fine_shifts"][foff[s]:foff[s + 1]], z["fine_means"][foff[s]:foff[s + 1]])
                 for s in range(int(z["n_scenes"]))]
    return z


def g10_scene(z, s):
    """(items as io.load_scene_items returns them, calibration inputs) of scene s."""
    items = []
    for i in np.flatnonzero(z["item_scene"] == s):
        cands = [z["cands"][c] for c in np.flatnonzero(z["cand_item"] == i)]
        items.append({"position": z["gts"][i], "noisy_candidates": cands, "context_lines": []})
    pred = [c for it in items for c in it["noisy_candidates"] if len(c) >= 2]
    gt = [it["position"] for it in items if it["position"] is not None and len(it["position"]) > 1]
    return items, pred, gt


def close(a, b, atol, rtol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= atol + rtol * np.abs(b))))


def test_g10_covers_the_cases(golden_dir):
    z = load_g10(golden_dir)
    assert (~z["valid"]).any() and z["bad_match"].any() and z["reversed"].any()
    assert (~z["item_has_pos"]).any() and (z["gt_len"] == 1).any() and (z["gt_len"] == 2).any()
    assert (z["cand_len"] == 1).any() and (~z["cal_done"]).any()
    assert (z["crop_start"][z["valid"]] == 0).any()
    last = [z["crop_end"][r] == z["gt_len"][z["row_item"][r]] - 1 for r in np.flatnonzero(z["valid"])]
    assert any(last)
    assert np.abs(z["gt_v"]).max() > 1e6                                    # the UTM-sized scene
    assert os.path.getsize(os.path.join(golden_dir, "g10_scene_metrics.npz")) <= 256 * 1024


def test_restatement_matches_reference_lines(golden_dir):
    z = load_g10(golden_dir)
    for r in range(len(z["valid"])):
        got = line_metrics_ref(z["noisy"][r], z["refined"][r], z["gts"][z["row_item"][r]])
        assert got["valid"] == z["valid"][r], r
        assert (got["crop_start"], got["crop_end"], got["reversed"]) == \
            (z["crop_start"][r], z["crop_end"][r], z["reversed"][r]), r
        assert got["bad_match"] == z["bad_match"][r], r
        assert close(got["resampled_gt"], z["resampled_gt"][r], 1e-12, 1e-12), r
        for k in M_KEYS:
            assert close(got[k], z[k][r], 1e-12, 1e-12), (r, k, got[k], z[k][r])


def test_restatement_matches_reference_calibration(golden_dir):
    z = load_g10(golden_dir)
    for s in range(int(z["n_scenes"])):
        _, pred, gt = g10_scene(z, s)
        assert z["cal_done"][s] == (len(pred) > 0 and len(gt) > 0)
        if not z["cal_done"][s]:
            continue
        cm = sweep_ref(np.vstack(pred), np.vstack(gt), coarse_grid())
        assert np.array_equal(coarse_grid(), z["coarse_shifts"])
        assert close(cm, z["coarse_means"][s], 0.0, 1e-12)
        best, off = pick(coarse_grid(), cm)
        fine_shifts, fine_means = z["fine"][s]
        assert np.array_equal(fine_grid(*off), fine_shifts)
        fm = sweep_ref(np.vstack(pred), np.vstack(gt), fine_shifts)
        assert close(fm, fine_means, 0.0, 1e-12)
        best, off = pick(fine_shifts, fine_means, *pick(z["coarse_shifts"], z["coarse_means"][s]))
        assert best == z["cal_best"][s] and off == (z["cal_dx"][s], z["cal_dy"][s])


def test_metrics_refuse_to_run_without_gpu(monkeypatch):
    from pointnet_refine_amd import metrics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    line = np.zeros((1, 32, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.line_metrics(line, line, [np.zeros((2, 3))])
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.shift_sweep(np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((1, 2)))
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.calibrate_alignment([np.zeros((2, 3))], [np.ones((2, 3))])
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.evaluate_scene(None, np.zeros((0, 4), np.float32), [])
    assert metrics.calibrate_alignment([], [np.ones((2, 3))]) == ((0, 0), 999.0)     # the reference's early exit
