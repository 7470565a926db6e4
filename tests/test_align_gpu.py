"""Paint alignment on the GPU (csrc/prh_align.hpp through pointnet_refine_amd.align) against the
restatement of the rule in _align_oracle.py.  Both tables - score, hits - are compared with the
oracle as bits: the rule's sums are integers, so there is nothing to tolerate.  The designed cases
come from the fixture g19 (stored inputs, stored results); the seeded ones from _align_cases.py,
whose oracle results are computed once per process.  Then the gap itself, end to end: a detector
drive whose lines lie (0.3, 0.44) m from the paint in every ego frame.

The end-to-end bounds are test_align_cpu's, met there by the numpy restatement on the same generator
and seed: along-lane |dx| <= 0.02 m (one fine step) and the fused y within 0.04 m of the lanes (the
0.02 m near-best bias of the rule's step 9, half a fine step, 0.01 m for sampling); every frame's
shift equals the restatement's as bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _align_cases as C
import _align_oracle as O
from pointnet_refine_amd import _lib as L
from pointnet_refine_amd import align as AL
from pointnet_refine_amd import fuse as F
from pointnet_refine_amd import link as LK
from pointnet_refine_amd import predictions as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(c, points=None, **more):
    res = AL.paint_scores(c["points"] if points is None else points, c["slice_offsets"], c["lines"], c["shifts"],
                          c["shift_offsets"], **dict(c["kw"], **more))
    assert sorted(res) == ["hits", "score"] and all(res[k].is_cuda and res[k].dtype == torch.int64 for k in C.KEYS)
    return {k: res[k].cpu().numpy() for k in C.KEYS}


def _same_bits(got, want, what):
    for k in C.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, (what, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])


@pytest.mark.parametrize("name", C.FIXTURE_CASES)
def test_fixture_cases_as_bits(golden_dir, name):
    """hits: d2 == r2, on the line, one ulp outside, a zero-length segment, a line of one vertex,
    non-finite x y z I, qi == 0, a point in two tubes; tiles: 0 / 1 / 63 / 64 / 65 / 257 candidates
    under 16 / 1 / 15 / 16 / 17 / 17 shifts - at cell 0.5, 1 and 4 m."""
    g = np.load(os.path.join(golden_dir, "g19_paint_align.npz"))
    c = C.case(name)
    assert np.array_equal(C.bits(g[f"{name}_points"]), C.bits(c["points"]))
    assert np.array_equal(C.bits(g[f"{name}_vertices"]), C.bits(C.csr(c["lines"])[0]))
    want = {k: g[f"{name}_{k}"] for k in C.KEYS}
    _same_bits(_run(c), want, name)
    for cell in (0.5, 1.0, 4.0):
        _same_bits(_run(c, cell=cell), want, f"{name} cell = {cell}")


def test_segment_tiles_as_bits():
    """prh_align_tile() and prh_align_tile() + 1 segments in a slice, a line that straddles the tile,
    hits on the last slot of the first tile and on the first of the second."""
    assert L.lib().prh_align_tile() == C.TILE and L.lib().prh_align_max_shifts() == AL.MAX_SHIFTS
    _same_bits(_run(C.case("segtile")), C.expected("segtile"), "segtile")


def test_ragged_slices_order_and_dtype():
    """Six slices (an empty one, lines without points, points without lines, two tables); the points
    of every slice shuffled; float32 points of equal value; points on the device; S = 1."""
    c = C.case("ragged")
    want = C.expected("ragged")
    _same_bits(_run(c), want, "ragged")
    for cell in (0.5, 4.0):
        _same_bits(_run(c, cell=cell), want, f"ragged cell = {cell}")
    rng = np.random.default_rng(5)
    shuffled = c["points"].copy()
    so = c["slice_offsets"]
    for s in range(len(so) - 1):
        shuffled[so[s]:so[s + 1]] = shuffled[so[s]:so[s + 1]][rng.permutation(so[s + 1] - so[s])]
    _same_bits(_run(c, points=shuffled), want, "shuffled")
    f32 = c["points"].astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), c["points"])       # the case's values are float32 values
    _same_bits(_run(c, points=f32), want, "float32")
    _same_bits(_run(c, points=torch.from_numpy(f32).cuda()), want, "float32 on the device")
    _same_bits(_run(c, points=torch.from_numpy(c["points"]).cuda()), want, "float64 on the device")
    floor = O.paint_scores(c["points"], so, c["lines"], c["shifts"], c["shift_offsets"], intensity_floor=20.0)
    _same_bits(_run(c, intensity_floor=20.0), floor, "floor 20")
    ko = c["shift_offsets"]
    one = {"points": c["points"][so[4]:so[5]], "slice_offsets": np.array([0, so[5] - so[4]]), "kw": {},
           "lines": [c["lines"][4]], "shifts": c["shifts"][ko[4]:ko[5]], "shift_offsets": np.array([0, ko[5] - ko[4]])}
    _same_bits(_run(one), {k: want[k][ko[4]:ko[5]] for k in C.KEYS}, "S = 1")


def test_empty_inputs_and_validation():
    z = AL.paint_scores(np.zeros((0, 4)), [0], [], np.zeros((0, 2)), [0])
    assert all(z[k].shape == (0,) for k in C.KEYS)
    line = [np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])]
    z = AL.paint_scores(np.zeros((0, 4)), [0, 0], [line], np.zeros((1, 2)), [0, 1])
    assert z["score"].cpu().tolist() == [0] and z["hits"].cpu().tolist() == [0]
    z = AL.paint_scores(np.array([[0.5, 0.0, 0.0, 9.0]]), [0, 1], [line], np.zeros((0, 2)), [0, 0])
    assert z["score"].shape == (0,)
    c = C.case("hits")
    for bad in ({"radius": 0.0}, {"radius": 1.5}, {"cell": 0.0}, {"cell": np.inf}, {"intensity_floor": np.nan}):
        with pytest.raises(ValueError):
            _run(c, **bad)
    args = (c["points"], c["slice_offsets"], c["lines"], c["shifts"], c["shift_offsets"])
    with pytest.raises(ValueError):
        AL.paint_scores(c["points"][:, :3], *args[1:])
    with pytest.raises(ValueError):
        AL.paint_scores(c["points"].astype(np.float16), *args[1:])
    with pytest.raises(ValueError):
        AL.paint_scores(c["points"], [0, 3], *args[2:])
    with pytest.raises(ValueError):
        AL.paint_scores(*args[:2], c["lines"] + [[]], *args[3:])                     # a list of lines too many
    with pytest.raises(ValueError):
        AL.paint_scores(*args[:2], [[np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]])]], *args[3:])
    with pytest.raises(ValueError):
        AL.paint_scores(*args[:2], [[np.array([[0.0, 0.0, 0.0], [2e6, 0.0, 0.0]])]], *args[3:])
    with pytest.raises(ValueError):
        AL.paint_scores(*args[:3], c["shifts"] * 2.0, args[4])                       # |component| = 6
    with pytest.raises(ValueError):
        AL.paint_scores(*args[:3], c["shifts"][:, :1], args[4])
    with pytest.raises(ValueError):
        AL.paint_scores(*args[:3], c["shifts"], [0, 2])
    with pytest.raises(ValueError):
        AL.paint_scores(*args[:3], np.zeros((AL.MAX_SHIFTS + 1, 2)), [0, AL.MAX_SHIFTS + 1])
    with pytest.raises(RuntimeError):
        AL.paint_scores(torch.from_numpy(c["points"]), *args[1:])                    # a CPU tensor
    for bad in ({"scope": "lane"}, {"max_shift": 0.0}, {"max_shift": 3.95}, {"max_shift": 3.5}, {"keep": (65, 64)},
                {"min_points": 0}):
        with pytest.raises(ValueError):
            AL.align_lines(c["points"], c["slice_offsets"], c["lines"], **bad)
    # the library's own limits
    lib = L.lib()
    assert lib.prh_align_score(None, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, 2.0, None, 0, None) != 0
    assert "radius" in lib.prh_last_error().decode()
    assert lib.prh_align_select_count(None, 1, None, 0, 0, None, None, None, None, 0, 0.0, 0.0, None, 0, None) != 0


def test_overflow_of_candidate_line_pairs():
    """2^20 candidates under 2^11 lines (all but one of a single vertex): 2^31 pairs in one slice."""
    n = 1 << 20
    pts = np.zeros((n, 4), dtype=np.float32)
    pts[:, 0] = np.linspace(0.0, 8.0, n, dtype=np.float32)
    pts[:, 3] = 30.0
    lines = [[np.array([[0.0, 0.0, 0.0], [8.0, 0.0, 0.0]])] + [np.array([[1.0, 1.0, 0.0]])] * ((1 << 11) - 1)]
    with pytest.raises(OverflowError):
        AL.paint_scores(pts, [0, n], lines, np.zeros((1, 2)), [0, 1])


@pytest.mark.parametrize("scope", ["frame", "drive"])
def test_align_lines_is_two_stages_and_the_picks(scope):
    f = C.small_frames()
    lines = [[v.copy() for v in ls] for ls in f["lines"]]
    shifted, rep = AL.align_lines(f["points"], f["slice_offsets"], lines, min_points=8, scope=scope)
    shifts, aligned, zero, best = O.align(f["points"], f["slice_offsets"], f["lines"], min_points=8, scope=scope)
    assert sorted(rep) == ["candidates", "frames", "frames_aligned", "frames_unaligned", "score_best", "score_zero", "shifts"]
    assert rep["shifts"].dtype == np.float64 and np.array_equal(C.bits(rep["shifts"]), C.bits(shifts))
    assert rep["frames"] == 3 and rep["frames_aligned"] == sum(aligned) and rep["frames_unaligned"] == 3 - sum(aligned)
    assert rep["score_zero"].tolist() == zero and rep["score_best"].tolist() == best and rep["score_zero"].dtype == np.int64
    assert 48 <= rep["candidates"] <= len(f["points"])          # the paint of the first two frames at least
    for s in range(3):
        for got, src in zip(shifted[s], f["lines"][s]):
            want = src.copy()
            want[:, 0] = want[:, 0] + shifts[s, 0]
            want[:, 1] = want[:, 1] + shifts[s, 1]
            assert np.array_equal(C.bits(got), C.bits(want)) and np.array_equal(got[:, 2], src[:, 2])
            assert np.array_equal(lines[s][0], src)             # the caller's lines are not written to
    if scope == "frame":
        assert aligned == [True, False, False] and abs(shifts[0, 1] - 0.25) <= 0.04
    else:
        assert np.array_equal(shifts[0], shifts[1]) and np.array_equal(shifts[0], shifts[2])
    empty, rep0 = AL.align_lines(np.zeros((0, 4)), [0], [])
    assert empty == [] and rep0["frames"] == 0 and rep0["shifts"].shape == (0, 2) and rep0["candidates"] == 0


# ------------------------------------------------------------------ a detector run beside the paint
def _write_offset_drive(root, pose_z=0.0, pitch=0.0):
    """_align_cases.paint_drive as files: merged.pcd, pose/*.json, a results JSON whose pixels are the
    two lanes moved by (0.3, 0.44) m in each ego frame, and the lanes as GT."""
    from pointnet_refine_amd.pcd import write_pcd_host
    cloud, poses, pixels = C.paint_drive(pose_z, pitch)
    drive = root / "drive"
    (drive / "pose").mkdir(parents=True)
    write_pcd_host(str(drive / "merged.pcd"), cloud)
    results = {}
    for k, pose in enumerate(poses):
        ts = 1000 + k
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": pose[3], "qy": pose[4], "qz": pose[5],
                   "qw": pose[6]}, open(drive / "pose" / f"{ts}.json", "w"))
        results[f"cam/{ts}.jpg"] = {"pred_instances": [{"data": px.tolist(), "score": 0.9} for px in pixels[k]]}
    json.dump(results, open(root / "results.json", "w"))
    F.write_map_json(str(root / "gt.json"), [[np.array([[-10.0, y, 0.0], [140.0, y, 0.0]])] for y in C.LANE_Y],
                     categories=["lane", "lane"])
    return drive, poses


def _zero_head_model():
    from pointnet_refine_amd.model import LineRefineNet
    from oracle import procedural as P
    m = LineRefineNet()
    m.load_state_dict(P.linerefine_state_dict(0))
    with torch.no_grad():
        for branch in m.reg_branches:
            branch[2].weight.zero_()
            branch[2].bias.zero_()
    return m


def _lane_errors(fused):
    out = []
    for parts in fused:
        y = np.concatenate([p[:, 1] for p in parts])
        lane = C.LANE_Y[int(np.argmin([abs(float(y.mean()) - v) for v in C.LANE_Y]))]
        out.append((float(np.abs(y - lane).min()), float(np.abs(y - lane).max())))
    return out


def _same_result(a, b):
    ra, rb = dict(a["report"]), dict(b["report"])
    for k in ("align_shifts", "align_score_zero", "align_score_best"):
        assert np.array_equal(C.bits(ra.pop(k)), C.bits(rb.pop(k))), k
    assert ra == rb and a["pieces"].tobytes() == b["pieces"].tobytes() and len(a["fused"]) == len(b["fused"])
    assert all(x.tobytes() == y.tobytes() for p, q in zip(a["fused"], b["fused"]) for x, y in zip(p, q))


def test_refine_predictions_needs_the_alignment_and_gets_it(tmp_path):
    drive, poses = _write_offset_drive(tmp_path)
    model = _zero_head_model().cuda().eval()
    args = (model, str(drive), str(tmp_path / "results.json"))
    plain = LK.refine_predictions(*args)
    assert not any(k.startswith("align_") for k in plain["report"]) and len(plain["fused"]) == 2
    for near, far in _lane_errors(plain["fused"]):
        print("without align: fused |y - lane| from", near, "to", far)
        assert near > 0.4                                       # the gap: the whole map lies beside the paint
    res = LK.refine_predictions(*args, align=True)
    rep = res["report"]
    print({k: v for k, v in rep.items() if k.startswith("align_")})
    assert rep["align_frames"] == rep["align_frames_aligned"] == 4 and rep["align_frames_unaligned"] == 0
    assert rep["pieces"] == 8 and rep["clusters_kept"] == 2 and len(res["fused"]) == 2
    # the restatement over the very slices refine_predictions cut
    scenes = PR.predictions_to_scenes(str(drive), str(tmp_path / "gt.json"), str(tmp_path / "results.json"), verbose=False)
    preds = [[PR.pixel_to_ego(px) for px in fr["pixels"]] for fr in PR.load_results(str(tmp_path / "results.json"))]
    want, aligned, zero, best = O.align(scenes["points"].cpu().numpy(), scenes["offsets"].cpu().numpy(), preds,
                                        scores=C.paint_scores_np)
    assert aligned == [True] * 4 and np.array_equal(C.bits(rep["align_shifts"]), C.bits(want))
    assert rep["align_score_zero"].tolist() == zero and rep["align_score_best"].tolist() == best
    assert np.abs(rep["align_shifts"][:, 0]).max() <= C.BOUND_DX
    for near, far in _lane_errors(res["fused"]):
        print("with align: fused |y - lane| from", near, "to", far)
        assert far <= C.BOUND_Y
    _same_result(LK.refine_predictions(*args, align=True, batched=True), res)
    one = LK.refine_predictions(*args, align=True, align_scope="drive")
    sh = one["report"]["align_shifts"]
    assert sh.shape == (4, 2) and all(np.array_equal(C.bits(sh[0]), C.bits(sh[k])) for k in range(4))
    assert one["report"]["align_frames_aligned"] == 4 and abs(sh[0, 0]) <= C.BOUND_DX
    assert all(far <= C.BOUND_Y for _, far in _lane_errors(one["fused"]))


def test_lift_and_align_on_the_raised_drive(tmp_path):
    """Poses 1.7 m above the road, pitched by 0.02 rad: the distances are 3-D, so without the lift
    no bright point is near a line; with both the map lies on the lanes."""
    drive, _ = _write_offset_drive(tmp_path, 1.7, 0.02)
    model = _zero_head_model().cuda().eval()
    args = (model, str(drive), str(tmp_path / "results.json"))
    flat = LK.refine_predictions(*args, align=True)
    assert flat["report"]["align_frames_aligned"] == 0 and flat["report"]["pieces"] == 0
    res = LK.refine_predictions(*args, lift=True, align=True)
    rep = res["report"]
    print({k: v for k, v in rep.items() if k.startswith("align_")})
    assert rep["lift_lines_lifted"] == 8 and rep["align_frames_aligned"] == 4 and rep["pieces"] == 8
    assert np.abs(rep["align_shifts"][:, 0]).max() <= C.BOUND_DX and len(res["fused"]) == 2
    for near, far in _lane_errors(res["fused"]):
        print("raised, lift and align: fused |y - lane| from", near, "to", far)
        assert far <= C.BOUND_Y


def test_example_aligns(tmp_path):
    drive, _ = _write_offset_drive(tmp_path)
    ckpt = tmp_path / "model.pth"
    torch.save(_zero_head_model().state_dict(), ckpt)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_predictions.py"), str(drive),
                          str(tmp_path / "results.json"), "--checkpoint", str(ckpt), "--out", str(tmp_path / "map.json"),
                          "--align"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "PAINT ALIGN  4 of 4 frames" in out.stdout and "2 clusters" in out.stdout


def test_prediction_scenes_carry_the_aligned_xy(tmp_path):
    from pointnet_refine_amd import drive as D
    drive, _ = _write_offset_drive(tmp_path)
    args = (str(drive), str(tmp_path / "gt.json"), str(tmp_path / "results.json"))
    plain = PR.predictions_to_scenes(*args, str(tmp_path / "plain"), verbose=False)
    again = PR.predictions_to_scenes(*args, str(tmp_path / "again"), verbose=False, align=False)
    moved = PR.predictions_to_scenes(*args, str(tmp_path / "moved"), verbose=False, align=True)
    names = sorted(os.listdir(tmp_path / "plain"))
    assert len(names) == 8 and names == sorted(os.listdir(tmp_path / "again")) == sorted(os.listdir(tmp_path / "moved"))
    for n in names:
        a, b = open(tmp_path / "plain" / n, "rb").read(), open(tmp_path / "again" / n, "rb").read()
        assert a == b, n                                        # align=False: byte-identical files
        if n.endswith(".pcd"):
            assert a == open(tmp_path / "moved" / n, "rb").read(), n
    assert "align" not in plain and "align" not in again and moved["align"]["frames_aligned"] == 4
    shifts = moved["align"]["shifts"]
    preds = [[PR.pixel_to_ego(px) for px in fr["pixels"]] for fr in PR.load_results(args[2])]
    for f, ts in enumerate(moved["frames"]):
        items = json.load(open(tmp_path / "moved" / f"{ts}.json"))["items"]
        plain_items = json.load(open(tmp_path / "plain" / f"{ts}.json"))["items"]
        assert len(items) == len(plain_items) == 2
        for i, it in enumerate(items):
            want = preds[f][i].copy()
            want[:, 0] = want[:, 0] + shifts[f, 0]
            want[:, 1] = want[:, 1] + shifts[f, 1]
            assert it["noisy_candidates"] == [D.xyz_dicts(want)]
            assert [p["z"] for p in it["noisy_candidates"][0]] == [p["z"] for p in plain_items[i]["noisy_candidates"][0]]
            assert it["noisy_candidates"] != plain_items[i]["noisy_candidates"]
            assert {k: v for k, v in it.items() if k != "noisy_candidates"} == \
                {k: v for k, v in plain_items[i].items() if k != "noisy_candidates"}
        assert np.array_equal(moved["matches"][f], plain["matches"][f])
