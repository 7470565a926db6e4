"""Writes tests/golden/g15_map_fusion.npz from tests/_fuse_oracle.py (the rule of
include/pointnet_refine_hip.h, "Map fusion - the rule", restated in numpy).  The reference has no
map fusion, so the fixture holds what the rule gives.  Not collected by pytest.

    python tests/make_golden_g15_map_fusion.py

3 poses 25 m apart with yaw and a small pitch, 400 km / 3,200 km from zero; 4 curved carriers of
uneven vertex spacing; 40 pieces of 32 points with 5 cm noise, shuffled, three or four per carrier
and pose, some reaching beyond the carrier's ends, one running against its carrier and one doubling
back.  The maker asserts the conditions under which the rule's decisions are well-posed, and
tests/test_fuse_gpu.py restates them on the stored arrays:
  - every node position is at least 1e-6 m away from every s of every piece, unless that s was
    clamped exactly to 0 or cum_total (exact on both sides);
  - every point's best segment beats every segment not next to it by at least 1e-6 m^2 in d2."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fuse_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g15_map_fusion.npz")
STEP, M, NOISE, MARGIN = 0.5, 32, 0.05, 1e-6


def make_inputs(seed=15):
    rng = np.random.default_rng(seed)
    base = np.array([400123.0, 3200456.0, 52.0])
    poses = O.make_poses(3, base, rng)
    lines = [O.curved_carrier(n, base + [-22.0, 0.0, -1.5], rng, length, lat)
             for n, length, lat in ((40, 95.0, -5.4), (57, 88.0, -1.8), (80, 97.0, 1.8), (33, 70.0, 5.4))]
    pieces, piece_line, piece_pose = [], [], []
    for l, v in enumerate(lines):
        total = O.carrier_cum(v)[-1]
        for k in range(3):
            centre = 22.0 + 25.0 * k
            for r in range(4 if (l + k) % 3 == 0 else 3):
                a = centre - rng.uniform(17.0, 27.0)
                b = centre + rng.uniform(17.0, 27.0)
                if b > total + 4.0:
                    b = total + rng.uniform(1.0, 4.0)
                sv = np.linspace(a, b, M)
                if (l, k, r) == (1, 1, 0):
                    sv = sv[::-1].copy()                                      # against the carrier
                if (l, k, r) == (2, 2, 1):
                    sv = np.concatenate([sv[:20], sv[19] - (sv[1:13] - sv[0])])  # doubles back
                pieces.append(O.make_piece(v, poses[k], sv, rng, NOISE))
                piece_line.append(l)
                piece_pose.append(k)
    order = rng.permutation(len(pieces))
    return (lines, np.stack(pieces)[order], np.array(piece_line, dtype=np.int64)[order],
            np.array(piece_pose, dtype=np.int64)[order], poses)


def main():
    lines, pieces, piece_line, piece_pose, poses = make_inputs()
    r = O.fuse(lines, pieces, piece_line, piece_pose, poses, STEP)
    shifted = [l - r["origin"] for l in lines]
    cums = [O.carrier_cum(v) for v in shifted]
    node_m, seg_m = O.margins(shifted, cums, r["world_shifted"], piece_line, r["s"], STEP)
    print(f"{len(pieces)} pieces, {len(r['C'])} nodes, {int((r['C'] > 0).sum())} used, largest C {int(r['C'].max())}, "
          f"node margin {node_m:.3g} m, segment margin {seg_m:.3g} m^2")
    assert node_m >= MARGIN and seg_m >= MARGIN
    assert np.abs(r["world_shifted"]).max() < 2000.0
    off = np.zeros(len(lines) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(l) for l in lines])
    np.savez_compressed(OUT, line_vertices=np.concatenate(lines), line_offsets=off, pieces=pieces, piece_line=piece_line,
                        piece_pose=piece_pose, poses=poses, step=np.float64(STEP), origin=r["origin"], world=r["world"],
                        s=r["s"], d=r["d"], seg=r["seg"], X=r["X"], W=r["W"], C=r["C"], spread=r["spread"],
                        node_offsets=r["offsets"],
                        fused_vertices=np.concatenate([p for f in r["fused"] for p in f]),
                        fused_sizes=np.array([len(p) for f in r["fused"] for p in f], dtype=np.int64),
                        fused_line=np.array([l for l, f in enumerate(r["fused"]) for _ in f], dtype=np.int64))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
