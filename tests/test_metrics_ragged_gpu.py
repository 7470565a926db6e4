"""The ragged evaluation on the GPU: prh_shift_sweep_ragged against one prh_shift_sweep call per
problem (bitwise) and against the numpy restatement, calibrate_alignments against
calibrate_alignment, evaluate_scenes against one evaluate_scene call per scene, and
SceneSampleStream(ragged=True) against ragged=False (byte for byte)."""
import functools

import numpy as np
import pytest
import torch

import test_metrics_cpu as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (256, 512, 16), (257, 513, 17), (300, 1, 5), (255, 511, 15), (1000, 777, 37), (130, 515, 600)]
ORIGIN = np.array([4e5, 5e6, 30.0])                                  # UTM-sized, as test_shift_sweep_matches_restatement


# ------------------------------------------------------------------ 1. the sweep, bitwise
def _sweep_problems():
    """Every tile edge twice: problem 7 + k shares problem k's GT set and has its predictions permuted."""
    rng = np.random.default_rng(101)
    preds, gts, shifts = [], [], []
    for n_pred, n_gt, n_shift in SHAPES:
        preds.append(rng.uniform(-30, 30, (n_pred, 3)) * [1, 1, 0.05] + ORIGIN)
        gts.append(rng.uniform(-30, 30, (n_gt, 3)) * [1, 1, 0.05] + ORIGIN)
        shifts.append(rng.uniform(-20, 20, (n_shift, 2)).round(1))
    for k in range(len(SHAPES)):
        preds.append(preds[k][rng.permutation(len(preds[k]))])
        shifts.append(rng.uniform(-20, 20, (SHAPES[k][2], 2)).round(1))
    return preds, gts, shifts, np.concatenate([np.arange(len(SHAPES))] * 2)


def test_ragged_sweep_is_bitwise_the_per_problem_sweep():
    from pointnet_refine_amd.metrics import shift_sweep, shift_sweep_ragged
    preds, gts, shifts, gt_index = _sweep_problems()
    got = shift_sweep_ragged(preds, gts, shifts, gt_index)
    assert len(got) == 14
    for p in range(14):
        one = shift_sweep(preds[p], gts[gt_index[p]], shifts[p])
        assert got[p].shape == (len(shifts[p]),) and got[p].dtype == np.float64
        assert np.array_equal(got[p], one), (p, np.flatnonzero(got[p] != one))
        want = R.sweep_ref(preds[p], gts[gt_index[p]], shifts[p])
        assert R.close(got[p], want, 0.0, 1e-12), (p, np.abs(got[p] / want - 1).max())
    again = shift_sweep_ragged([torch.from_numpy(a).cuda() for a in preds], [torch.from_numpy(a).cuda() for a in gts],
                               shifts, gt_index)
    twice = shift_sweep_ragged(preds, gts, shifts, gt_index)
    for p in range(14):
        assert got[p].tobytes() == again[p].tobytes() == twice[p].tobytes(), p
    # without gt_index problem p uses set p; a problem without points is left out and shifts nobody else
    own = shift_sweep_ragged(preds[:3] + [np.zeros((0, 3))] + preds[4:7], gts, shifts[:7])
    for p in range(7):
        assert np.isnan(own[p]).all() and own[p].shape == (5,) if p == 3 else np.array_equal(own[p], got[p]), p


def test_ragged_sweep_takes_more_items_than_a_2d_grid():
    """70,000 one-point problems: a leftover blockIdx.y or a 16-bit tile index cannot reach them."""
    from pointnet_refine_amd.metrics import shift_sweep, shift_sweep_ragged
    n = 70000
    rng = np.random.default_rng(102)
    pred = rng.uniform(-30, 30, (n, 3)) * [1, 1, 0.05] + ORIGIN
    gt = rng.uniform(-30, 30, (n, 3)) * [1, 1, 0.05] + ORIGIN
    shifts = rng.uniform(-20, 20, (n, 2)).round(1)
    got = shift_sweep_ragged(list(pred[:, None, :]), list(gt[:, None, :]), list(shifts[:, None, :]))
    got = np.concatenate(got)
    assert got.shape == (n,)
    want = R.norm_rows(pred + np.column_stack([shifts, np.zeros(n)]) - gt)
    assert R.close(got, want, 0.0, 1e-12), np.abs(got / want - 1).max()
    for p in (0, n - 1, int(rng.integers(1, n - 1))):
        assert np.array_equal(got[p:p + 1], shift_sweep(pred[p:p + 1], gt[p:p + 1], shifts[p:p + 1])), p
    # the same problem at three positions of one call gives the same bytes
    where = [0, 34567, n - 1]
    preds, gts, shs = list(pred[:, None, :]), list(gt[:, None, :]), list(shifts[:, None, :])
    big_p, big_g, big_s = _sweep_problems()[0][5], _sweep_problems()[1][5], _sweep_problems()[2][5]
    for w in where:
        preds[w], gts[w], shs[w] = big_p, big_g, big_s
    moved = shift_sweep_ragged(preds, gts, shs)
    one = shift_sweep(big_p, big_g, big_s)
    for w in where:
        assert np.array_equal(moved[w], one), w
    assert np.array_equal(moved[1][0], got[1])


# ------------------------------------------------------------------ 3. calibration
def _same_calibration(a, b):
    assert a[:2] == b[:2], (a[:2], b[:2])
    assert type(a[0][0]) is type(b[0][0]) and type(a[1]) is type(b[1])
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        assert np.array_equal(a[2][k][0], b[2][k][0]) and np.array_equal(a[2][k][1], b[2][k][1], equal_nan=True), k


def _synthetic_calibration(seed, shift):
    rng = np.random.default_rng(seed)
    gt, pred = [], []
    for i in range(5):
        x = np.sort(rng.uniform(-40, 40, int(rng.integers(5, 60))))
        line = np.stack([x, 4.0 * i + 0.3 * np.sin(x / 6.0), rng.normal(0, 0.05, len(x))], 1) + ORIGIN
        gt.append(line)
        for _ in range(2):
            pred.append(line[:: int(rng.integers(1, 3))] + [shift[0], shift[1], 0.0] + rng.normal(0, 0.05, 3))
    return pred, gt


def test_calibrate_alignments_equals_calibrate_alignment(golden_dir):
    from pointnet_refine_amd.metrics import calibrate_alignment, calibrate_alignments
    z = R.load_g10(golden_dir)
    problems, g10 = [], {}
    for s in range(int(z["n_scenes"])):
        _, pred, gt = R.g10_scene(z, s)
        g10[len(problems)] = s
        problems.append((pred, gt))
    problems.insert(2, ([], problems[0][1]))                          # an empty prediction list in the middle
    g10 = {(p if p < 2 else p + 1): s for p, s in g10.items()}
    problems.append(_synthetic_calibration(7, (3.3, -1.7)))
    problems.append(_synthetic_calibration(8, (-11.0, 6.4)))
    preds, gts = [p for p, _ in problems], [g for _, g in problems]
    got = calibrate_alignments(preds, gts, return_tables=True)
    plain = calibrate_alignments(preds, gts)
    assert got[2] == ((0, 0), 999.0, {}) and plain[2] == ((0, 0), 999.0)
    for p, (pred, gt) in enumerate(problems):
        _same_calibration(got[p], calibrate_alignment(pred, gt, return_tables=True))
        assert plain[p] == calibrate_alignment(pred, gt) == got[p][:2]
    # leaving the empty problem out changes nobody's result
    rest = calibrate_alignments(preds[:2] + preds[3:], gts[:2] + gts[3:], return_tables=True)
    for a, b in zip(rest, got[:2] + got[3:]):
        _same_calibration(a, b)
    # a shared GT list through gt_index: the same values
    shared = calibrate_alignments([preds[0], preds[1], preds[0], preds[4]], [gts[4], gts[0], gts[1]], gt_index=[1, 2, 1, 0])
    assert shared == [plain[0], plain[1], plain[0], plain[4]]
    # the synthetic shifts are found: half a fine step (0.1) plus the per-line jitter (0.05 sigma)
    for p, want in ((len(problems) - 2, (-3.3, 1.7)), (len(problems) - 1, (11.0, -6.4))):
        assert abs(plain[p][0][0] - want[0]) <= 0.4 and abs(plain[p][0][1] - want[1]) <= 0.4, plain[p]
    # the reference's values, to the bounds of test_calibrate_alignment_matches_reference
    for p, s in g10.items():
        if not z["cal_done"][s]:
            assert plain[p] == ((0, 0), 999.0)
            continue
        (dx, dy), best, tables = got[p]
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


# ------------------------------------------------------------------ 4. evaluate_scenes
KW = dict(num_context_points=256, crop_radius=0.5, batch_lines=7, seed=3)
EXACT = ("item_index", "candidate_index", "noisy", "calibration", "valid", "crop_start", "crop_end", "reversed",
         "resampled_gt")


def _scene(seed, n_cloud, gt=True, long_candidates=True):
    """A scene made like _synthetic_scene of test_metrics_gpu.py."""
    rng = np.random.default_rng(seed)
    items = []
    for i in range(6):
        n = int(rng.integers(4, 30))
        x = np.sort(rng.uniform(-20, 20, n))
        pos = np.stack([x, 3.5 * i + 0.2 * np.sin(x / 5.0), np.zeros(n)], 1)
        cands = []
        for k in range(3):
            nv = [1, 5, 12][(i + k) % 3] if long_candidates else 1
            cx = np.linspace(rng.uniform(-20, -5), rng.uniform(5, 20), nv)
            cands.append(np.stack([cx, 3.5 * i + 0.2 * np.sin(cx / 5.0) + rng.uniform(-0.4, 0.4),
                                   rng.normal(0, 0.02, nv)], 1))
        items.append({"position": pos if gt and i != 2 else None, "noisy_candidates": cands, "context_lines": []})
    if gt:
        items[4]["position"] = items[4]["position"][:1]               # a 1-vertex GT
    xyz = np.stack([rng.uniform(-22, 22, n_cloud), rng.uniform(-2, 20, n_cloud), rng.normal(0, 0.05, n_cloud)], 1)
    cloud = np.column_stack([xyz, rng.uniform(0, 60, n_cloud)]).astype(np.float32)
    return cloud, items


@functools.lru_cache(maxsize=None)
def _scenes():
    return [_scene(21, 30000), _scene(22, 3000, gt=False), _scene(23, 9000, long_candidates=False), _scene(24, 0),
            _scene(25, 12000)]


@functools.lru_cache(maxsize=None)
def _model(zero_head):
    from oracle import procedural as P
    from pointnet_refine_amd.model import LineRefineNet
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0))
    if zero_head:
        with torch.no_grad():
            for branch in m.reg_branches:
                branch[2].weight.zero_()
                branch[2].bias.zero_()
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _per_scene(zero_head):
    """One evaluate_scene call per scene: computed once per model, shared, never written to."""
    from pointnet_refine_amd.metrics import evaluate_scene
    return [evaluate_scene(_model(zero_head), cloud, items, **KW) for cloud, items in _scenes()]


@functools.lru_cache(maxsize=None)
def _ragged(zero_head, max_points=None):
    from pointnet_refine_amd.metrics import evaluate_scenes
    return evaluate_scenes(_model(zero_head), _scenes(), max_points=max_points, **KW)


def _same_field(a, b, key):
    if a is None or b is None or isinstance(a, tuple):
        assert a == b, (key, a, b)
    else:
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key


def test_evaluate_scenes_zero_head_is_evaluate_scene_exactly():
    want, got = _per_scene(True), _ragged(True)
    assert len(got) == 5
    for s in range(5):
        assert got[s].keys() == want[s].keys(), s
        for key in want[s]:
            _same_field(got[s][key], want[s][key], (s, key))
    rows = [len(d["item_index"]) for d in got]
    assert rows[2] == 0 and min(rows[0], rows[1], rows[3], rows[4]) > 0
    assert got[1]["calibration"] is None and got[2]["calibration"] is None and not got[1]["valid"].any()
    assert got[3]["calibration"] is not None and got[0]["valid"].any() and not got[0]["valid"].all()
    assert np.array_equal(got[0]["refined"], got[0]["noisy"])           # a zero head: no offset at all


def test_evaluate_scenes_procedural_model():
    from pointnet_refine_amd.metrics import calibrate_alignment, line_metrics, scene_rows
    want, got = _per_scene(False), _ragged(False)
    worst, moved = 0.0, 0.0
    for s, (_, items) in enumerate(_scenes()):
        for key in EXACT:
            _same_field(got[s][key], want[s][key], (s, key))
        assert got[s].keys() == want[s].keys()
        if len(got[s]["refined"]):
            worst = max(worst, float(np.abs(got[s]["refined"] - want[s]["refined"]).max()))
            moved = max(moved, float(np.abs(got[s]["refined"] - got[s]["noisy"]).max()))
        # the metric fields: line_metrics on the result's own lines
        _, _, gts, cal_gt = scene_rows(items)
        gt_index = np.array([-1 if g is None else r for r, g in enumerate(gts)], dtype=np.int64)
        own = line_metrics(got[s]["noisy"], got[s]["refined"], gts, gt_index)
        for key in own:
            _same_field(got[s][key], own[key], (s, key))
        if len(got[s]["refined"]) and cal_gt:
            assert got[s]["calibration_refined"] == calibrate_alignment(list(got[s]["refined"]), cal_gt), s
        else:
            assert got[s]["calibration_refined"] is None
    print(f"evaluate_scenes vs evaluate_scene: refined differs by at most {worst:.3e} m (offsets up to {moved:.3e} m)")
    assert moved > 1e-3                                               # the offsets are not zero here
    assert worst <= 2e-4


def test_evaluate_scenes_grouping_changes_no_exact_field():
    from pointnet_refine_amd.metrics import scene_groups
    clouds = [len(c) for s, (c, _) in enumerate(_scenes()) if s != 2]  # the scenes that have rows
    assert scene_groups(clouds, 14000) == [(0, 1), (1, 3), (3, 4)]
    for zero_head in (True, False):
        one, three = _ragged(zero_head), _ragged(zero_head, 14000)
        for s in range(5):
            for key in (one[s].keys() if zero_head else EXACT):
                _same_field(three[s][key], one[s][key], (s, key))
            if not zero_head and len(one[s]["refined"]):
                assert np.abs(three[s]["refined"] - one[s]["refined"]).max() <= 2e-4


def test_evaluate_scenes_takes_device_clouds_and_extra_columns():
    from pointnet_refine_amd.metrics import evaluate_scenes
    scenes = [(torch.from_numpy(c).cuda(), it) if s % 2 else (np.column_stack([c, np.ones(len(c), np.float32)]), it)
              for s, (c, it) in enumerate(_scenes())]
    got, want = evaluate_scenes(_model(True), scenes, **KW), _ragged(True)
    for s in range(5):
        for key in want[s]:
            _same_field(got[s][key], want[s][key], (s, key))
    assert evaluate_scenes(_model(True), [], **KW) == []


# ------------------------------------------------------------------ 5. the sample stream
def _write_root(root):
    from pointnet_refine_amd import drive
    rng = np.random.default_rng(31)
    for s in range(4):
        xyz = np.stack([rng.uniform(-25, 25, 2000), rng.uniform(-3, 12, 2000), rng.normal(0, 0.05, 2000)], 1)
        cloud = np.column_stack([xyz, rng.integers(0, 60, 2000)]).astype(np.float32)
        items = []
        for i in range(3):
            x = np.sort(rng.uniform(-24, 24, int(rng.integers(4, 20))))
            pos = np.stack([x, 3.5 * i + 0.2 * np.sin(x / 5.0 + s), np.zeros(len(x))], 1)
            cands = [pos + rng.normal(0, 0.2, 3) for _ in range(3)]
            items.append({"category": "lane", "attributes": {}, "points": pos, "noisy_candidates": cands})
        drive.write_scene(str(root / f"scene_{s}.pcd"), str(root / f"scene_{s}.json"), cloud, items, "0")
    return str(root)


@pytest.mark.parametrize("augment", [None, (0.1, 0.25)])
def test_ragged_stream_yields_the_same_bytes(tmp_path, augment, monkeypatch):
    from pointnet_refine_amd import io
    root = _write_root(tmp_path)
    calls = {"ragged": 0, "plain": 0}
    ragged_builder, plain_builder = io.build_contexts_ragged, io.build_contexts
    monkeypatch.setattr(io, "build_contexts_ragged",
                        lambda *a, **k: (calls.__setitem__("ragged", calls["ragged"] + 1), ragged_builder(*a, **k))[1])
    monkeypatch.setattr(io, "build_contexts",
                        lambda *a, **k: (calls.__setitem__("plain", calls["plain"] + 1), plain_builder(*a, **k))[1])
    for rank, world in ((0, 1), (1, 2)):
        kw = dict(num_context_points=256, batch_size=5, mix_scenes=3, seed=5, augment=augment, rank=rank, world_size=world)
        plain, ragged = io.SceneSampleStream(root, **kw), io.SceneSampleStream(root, ragged=True, **kw)
        assert len(plain) == len(ragged) == -(-(36 if augment is None else 24) // world)
        for epoch in (0, 1):
            plain.set_epoch(epoch)
            ragged.set_epoch(epoch)
            calls.update(ragged=0, plain=0)
            a = list(plain)
            assert calls["ragged"] == 0 and calls["plain"] >= 3
            n_plain = calls["plain"]
            calls.update(ragged=0, plain=0)
            b = list(ragged)
            assert calls["plain"] == 0 and 1 <= calls["ragged"] <= 2 < n_plain     # 4 scenes, groups of 3
            assert len(a) == len(b) == -(-len(plain) // 5)
            for x, y in zip(a, b):
                assert x.keys() == y.keys()
                for k in x:
                    assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), (rank, epoch, k)
    # one batch per scene: nothing to pool, ragged is ignored
    one = list(io.SceneSampleStream(root, num_context_points=256, batch_size=None, seed=5, augment=augment, ragged=True))
    ref = list(io.SceneSampleStream(root, num_context_points=256, batch_size=None, seed=5, augment=augment))
    assert len(one) == len(ref) == 4 and all(torch.equal(x["context"], y["context"]) for x, y in zip(one, ref))


# ------------------------------------------------------------------ the two command-line callers
def _run_example(name, argv, monkeypatch, capsys):
    import importlib.util
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", name)
    spec = importlib.util.spec_from_file_location("example_" + name[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", [path] + [str(a) for a in argv])
    capsys.readouterr()
    mod.main()
    return capsys.readouterr().out


def test_examples_print_the_same_with_batched(tmp_path, golden_dir, monkeypatch, capsys):
    """examples/evaluate_scenes.py and predictions_to_scenes.py --evaluate: --batched prints what the
    per-scene loop prints (a zero-head checkpoint: the two modes then agree in every digit)."""
    import json
    import test_predictions_cpu as RP
    from pointnet_refine_amd import drive
    data = tmp_path / "data"
    data.mkdir()
    for s, (cloud, items) in enumerate(_scenes()):
        if len(cloud) == 0:
            continue                                                  # an empty ASCII PCD is the readers' business, not this test's
        out = [{"category": "lane", "attributes": {}, "points": np.zeros((0, 3)) if it["position"] is None else it["position"],
                "noisy_candidates": it["noisy_candidates"]} for it in items]
        drive.write_scene(str(data / f"s{s}.pcd"), str(data / f"s{s}.json"), cloud, out, "0")
    ckpt = tmp_path / "zero_head.pth"
    torch.save({k: v.cpu() for k, v in _model(True).state_dict().items()}, ckpt)
    texts, dumps = [], []
    for flags in ([], ["--batched", "--max-points", 14000]):
        out_json = tmp_path / f"eval{len(flags)}.json"
        text = _run_example("evaluate_scenes.py", [data, "--checkpoint", ckpt, "--json", out_json] + flags, monkeypatch, capsys)
        texts.append([line.split(" | metric stage")[0] for line in text.splitlines()])
        d = json.load(open(out_json))
        d["summary"].pop("metric_rows_per_s")
        dumps.append(d)
    assert texts[0] == texts[1] and dumps[0] == dumps[1]
    assert sum(line.startswith("    Line ") for line in texts[0]) > 10
    assert sum(line.startswith("XXX SCENE CALIBRATION XXX") for line in texts[0]) == 2 and texts[0][-1].startswith("SUMMARY over")
    # prediction scenes of the g12 drive, scored per frame and in one call
    z = RP.load_g12(golden_dir)
    drive_dir, gt, results = RP._write_drive(z, str(tmp_path / "drive"))
    lines = []
    for flags in ([], ["--batched"]):
        text = _run_example("predictions_to_scenes.py", [drive_dir, gt, results, tmp_path / f"scenes{len(flags)}", "--evaluate", ckpt]
                            + flags, monkeypatch, capsys)
        lines.append([line for line in text.splitlines() if line.startswith("EVALUATION over")])
    assert len(lines[0]) == 1 and lines[0] == lines[1]
