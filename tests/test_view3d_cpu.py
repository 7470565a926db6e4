"""Host side of the 3-D views (pointnet_refine_amd.view3d): the oracle against its committed
fixture, the camera rows against their closed forms, the colour table against matplotlib, the
host-packed line segments against the oracle bit for bit, and the C ABI against its ctypes binding.
Every comparison of segments and words is of bits; camera rows are held to a few ulp."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _view3d_oracle as O
import make_golden_g14_view3d as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = np.finfo(np.float64).eps


def _view():
    from pointnet_refine_amd import view3d
    return view3d


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_oracle_reproduces_the_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "g14_view3d.npz"))
    got = M.golden(z["points"], z["cameras"])          # bitwise from the stored rows on: no libm in between
    fresh = M.golden()                                 # the rows themselves: to a few ulp of the eye distance
    assert np.abs(fresh["cameras"] - z["cameras"]).max() <= 4 * ULP * 10.0 and fresh["points"].shape == z["points"].shape
    assert sorted(z.files) == sorted(got)
    for k in z.files:
        a, b = z[k], got[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    assert os.path.getsize(os.path.join(golden_dir, "g14_view3d.npz")) < 200 * 1024
    # the fixture is not trivial: points and lines both show, and pixels stay empty
    pay = z["words"] & np.uint64(0xFFFFFFFF)
    filled = z["words"] != O.EMPTY
    assert (filled & (pay >= 0x01000000)).sum() > 300 and (filled & (pay < 0x01000000)).sum() > 100 and (~filled).sum() > 100


@pytest.mark.parametrize("elev,azim", [(30.0, -60.0), (0.0, 0.0), (90.0, 0.0), (-90.0, 90.0), (20.0, 60.0), (55.0, 200.0)])
def test_camera_rows_are_orthonormal_and_look_at_the_target(elev, azim):
    V = _view()
    target, dist = np.array([3.0, -2.0, 1.5]), 17.0
    row = V.orbit_camera(target, elev, azim, dist, fov=40.0, near=0.2, height=480, width=640)
    assert row.shape == (16,) and row.dtype == np.float64
    eye, r, u, f = row[0:3], row[3:6], row[6:9], row[9:12]
    tol = 4 * ULP
    for a in (r, u, f):
        assert abs(a @ a - 1.0) <= tol
    assert abs(r @ u) <= tol and abs(r @ f) <= tol and abs(u @ f) <= tol
    assert np.abs(np.cross(r, u) + f).max() <= tol               # right-handed: r x u = -f (the eye looks along f)
    assert np.abs(eye + dist * f - target).max() <= tol * dist
    assert abs(row[12] / ((480 / 2.0) / np.tan(np.radians(40.0) / 2.0)) - 1.0) <= tol and row[13] == 0.2 and row[14] == 0.0 and row[15] == 0.0
    ref = O.camera(target, elev, azim, dist, 480, fov=40.0, near=0.2)
    assert np.abs(row - ref).max() <= tol * dist
    o = V.orbit_camera(target, elev, azim, dist, ortho_scale=12.5, near=0.0, height=480, width=640)
    assert o[12] == 12.5 and o[14] == 1.0 and np.array_equal(o[:12], row[:12])


def test_camera_closed_forms_at_the_poles_and_axes():
    V = _view()
    c = np.array([1.0, 2.0, 3.0])
    want = {
        (0, 0): ([11, 2, 3], [0, 1, 0], [0, 0, 1], [-1, 0, 0]),
        (0, 90): ([1, 12, 3], [-1, 0, 0], [0, 0, 1], [0, -1, 0]),
        (90, 0): ([1, 2, 13], [0, 1, 0], [-1, 0, 0], [0, 0, -1]),
        (90, 90): ([1, 2, 13], [-1, 0, 0], [0, -1, 0], [0, 0, -1]),
        (-90, 0): ([1, 2, -7], [0, 1, 0], [1, 0, 0], [0, 0, 1]),
        (-90, 90): ([1, 2, -7], [-1, 0, 0], [0, 1, 0], [0, 0, 1]),
    }
    for (elev, azim), parts in want.items():
        row = V.orbit_camera(c, float(elev), float(azim), 10.0)
        assert np.abs(row[:12] - np.concatenate([np.asarray(p, dtype=np.float64) for p in parts])).max() <= 4 * ULP * 13, (elev, azim)
        assert np.isfinite(row).all()
    with pytest.raises(ValueError):
        V.orbit_camera(c, 0.0, 0.0, 10.0, near=0.0)
    with pytest.raises(ValueError):
        V.orbit_camera(c, 0.0, 0.0, 10.0, fov=180.0)


def test_fit_camera_holds_the_bounding_sphere():
    V = _view()
    lo, hi = np.array([-4.0, -1.0, 0.0]), np.array([10.0, 3.0, 2.0])
    for ortho in (False, True):
        row = V.fit_camera((lo, hi), 25.0, -40.0, ortho=ortho, height=300, width=400)
        centre, radius = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        xr, yu, d = O.view_space(corners, row)
        x, y = O.screen(xr, yu, d, row, 300, 400)
        assert (d >= row[13]).all() and (x >= 0).all() and (x <= 400).all() and (y >= 0).all() and (y <= 300).all()
        xr, yu, d = O.view_space(centre[None], row)
        x, y = O.screen(xr, yu, d, row, 300, 400)
        assert abs(x[0] - 200) < 1e-9 and abs(y[0] - 150) < 1e-9 and d[0] >= radius
    six = V.fit_camera([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], 25.0, -40.0, height=300, width=400)
    assert np.array_equal(six, V.fit_camera((lo, hi), 25.0, -40.0, height=300, width=400))


def test_viridis_table_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    V = _view()
    t = V.viridis_table()
    assert t.shape == (256, 4) and t.dtype == np.uint8
    assert np.array_equal(t, matplotlib.colormaps["viridis"](np.arange(256), bytes=True))


def test_tables_have_the_shape_resolve_takes():
    V = _view()
    for t in (V.viridis_table(), V.jet_table(), V.gray_table()):
        assert t.shape == (256, 4) and t.dtype == np.uint8 and (t[:, 3] == 255).all()
    assert tuple(V.viridis_table()[0]) == (68, 1, 84, 255) and tuple(V.viridis_table()[255]) == (253, 231, 36, 255)


def _pack_equals_oracle(lines, styles, cams, line_views=None):
    V = _view()
    segs, ids, st = V.pack_lines3d(lines, styles, cams, M.H, M.W, line_views)
    want_s, want_i = O.segments(lines, cams, M.H, M.W, line_views)
    assert segs.shape == want_s.shape and segs.dtype == np.float64 and ids.dtype == np.int32
    assert np.array_equal(bits(segs), bits(want_s)) and np.array_equal(ids, want_i)
    assert np.array_equal(bits(st), bits(np.array([O.style_row(s) for s in styles]).reshape(-1, 8)))
    return segs, ids


def test_pack_lines3d_equals_oracle_bit_for_bit():
    lines, styles, cams = M.lines_scene()
    cams[0, 13] = 2.5
    segs, ids = _pack_equals_oracle(lines, styles, cams)
    assert np.isfinite(segs).all() and len(segs) > 20
    # a line crossing the near plane: cut at d == near (wa or wb = 1 / near in the perspective view)
    s5 = segs[(ids[:, 0] == 5) & (ids[:, 1] == 0)]
    assert len(s5) == 1 and s5[0, 7] == 1.0 / 2.5 and s5[0, 6] < s5[0, 7]
    # a line wholly behind the camera gives no segment there
    assert not ((ids[:, 0] == 6) & (ids[:, 1] == 0)).any()
    # a single vertex: one zero-length segment per view that sees it
    s4 = segs[ids[:, 0] == 4]
    assert len(s4) == 3 and (s4[:, 0] == s4[:, 2]).all() and (s4[:, 1] == s4[:, 3]).all() and (s4[:, 4:6] == 0).all()
    # arc lengths run on from the first drawn vertex
    s1 = segs[(ids[:, 0] == 1) & (ids[:, 1] == 1)]
    assert len(s1) == 3 and s1[0, 4] == 0.0 and s1[1, 4] == s1[0, 5] and s1[2, 4] == s1[0, 5] + s1[1, 5]
    # orthographic views carry d itself
    xr, yu, d = O.view_space(lines[0], cams[1])
    s0 = segs[(ids[:, 0] == 0) & (ids[:, 1] == 1)]
    assert np.array_equal(s0[:, 6], d[:-1]) and np.array_equal(s0[:, 7], d[1:])


def test_pack_lines3d_per_line_views_and_edge_cases():
    lines, styles, cams = M.lines_scene()
    views = [[0], [1, 2], None, [2], [0, 1, 2], [0], [0], [2, 0], [1], []]
    segs, ids = _pack_equals_oracle(lines, styles, cams, views)
    assert set(map(tuple, ids[ids[:, 0] == 1])) == {(1, 1), (1, 2)} and not (ids[:, 0] == 9).any()
    # all lines behind every camera, and no lines at all
    behind = [np.array([c[0:3] - 2.0 * c[9:12], c[0:3] - 5.0 * c[9:12]]) for c in cams]
    for k, line in enumerate(behind):
        segs, ids = _pack_equals_oracle([line], styles[:1], cams[k:k + 1])
        assert segs.shape == (0, 8) and ids.shape == (0, 2)
    segs, ids = _pack_equals_oracle([], [], cams)
    assert segs.shape == (0, 8)
    V = _view()
    with pytest.raises(ValueError):
        V.pack_lines3d(lines[:2], styles[:1], cams, M.H, M.W)
    with pytest.raises(ValueError):
        V.pack_lines3d(lines[:1], styles[:1], cams, M.H, M.W, [[3]])


_CTYPES = {"int": C.c_int, "long long": C.c_longlong, "double": C.c_double, "float": C.c_float, "size_t": C.c_size_t,
           "unsigned": C.c_uint, "long": C.c_long}


def _c_type(text):
    text = re.sub(r"\bconst\b", "", text).strip()
    if "*" in text:
        return C.c_void_p
    words = text.split()
    if words[-1] not in ("int", "long", "double", "float", "size_t", "unsigned", "char"):
        words = words[:-1]                        # the parameter's name
    return _CTYPES[" ".join(words)]


def test_view_abi_and_binding_declare_the_same_signatures():
    from pointnet_refine_amd import _lib
    _lib.build()
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pointnet_refine_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decls = re.findall(r"^([a-z_ ]+?)\s+(prh_view_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
    names = [d[1] for d in decls]
    assert sorted(names) == sorted(n for n in _lib.EXPORTS if n.startswith("prh_view_")) and len(names) == 7
    for ret, name, params in decls:
        fn = getattr(lib, name)
        params = [] if params.strip() in ("void", "") else [_c_type(p) for p in params.split(",")]
        assert fn.restype is _c_type(ret + " x"), name
        assert list(fn.argtypes) == params, name

