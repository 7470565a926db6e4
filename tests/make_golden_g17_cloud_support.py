"""Writes tests/golden/g17_cloud_support.npz from tests/_support_oracle.py (the rule of
include/pointnet_refine_hip.h, "Cloud support - the rule", restated in Python floats).  The
reference has no counterpart of this stage, so the fixture holds what the rule gives.  Not
collected by pytest.

    python tests/make_golden_g17_cloud_support.py

Three curved lines of 9, 14 and 2 vertices, tilted in z, 400 km / 3,200 km from zero, and 2,500
float32 points around them with intensities in multiples of 1/4 (_support_cases.fixture_case).  The
maker asserts the conditions under which the rule's integers are well-posed, and
tests/test_support_gpu.py restates them from the oracle on the stored inputs:
  - every (point, line) pair has |d2 - r2| >= 1e-9 m^2;
  - every hit not clamped to the last node has s / step + 0.5 at least 1e-9 from an integer;
  - t * 65536, hz * 65536 and wI * 256 of every hit are at least 1e-8 from a half-integer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _support_cases as C  # noqa: E402
import _support_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g17_cloud_support.npz")
STEP, RADIUS = 0.5, 0.3


def main():
    lines, cloud = C.fixture_case()
    r = O.support(cloud, lines, STEP, RADIUS, C.FLOOR)
    m = r["margins"]
    print(f"{len(cloud)} points, {len(r['hits'])} hits, {len(r['acc'])} nodes, largest n {int(r['acc'][:, 0].max())}, "
          f"margins d2 {m['d2']:.3g} m^2, station {m['station']:.3g}, quantisation {m['quant']:.3g}, lead {m['lead']:.3g} m^2")
    C.assert_margins(m)
    off = np.zeros(len(lines) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(l) for l in lines])
    np.savez_compressed(OUT, line_vertices=np.concatenate(lines), line_offsets=off, cloud=cloud, step=np.float64(STEP),
                        radius=np.float64(RADIUS), intensity_floor=np.float64(C.FLOOR), origin=r["origin"], acc=r["acc"],
                        node_offsets=r["offsets"])
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
