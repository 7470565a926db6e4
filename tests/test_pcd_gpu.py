"""PCD codec on the GPU (csrc/prh_pcd.hpp).  The expected text is Python's own '%' formatting - the
rule np.savetxt applies - and the expected values are np.loadtxt(dtype=float32)'s, compared as bit
patterns.  Everything goes through the strict device functions, so a host fallback cannot pass."""
import io as _io
import os
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest
import torch

import test_drive_cpu as R

pytestmark = pytest.mark.gpu

FMT = "%.4f %.4f %.4f %d\n"


def _pcd():
    from pointnet_refine_amd import pcd
    return pcd


def _expect(rows):
    return b"".join((FMT % tuple(r)).encode() for r in np.asarray(rows, dtype=np.float64).reshape(-1, 4))


def _text(points, offsets=None):
    text, boff = _pcd().format_rows(points, offsets)
    assert text.dtype == torch.uint8 and text.is_cuda and boff.dtype == torch.int64
    return text.cpu().numpy().tobytes(), boff.cpu().numpy()


def _random_rows(n, seed):
    """Half float32-exact, half full doubles, magnitudes 10^U(-8, 11), inside the device domain."""
    rng = np.random.default_rng(seed)
    a = rng.choice([-1.0, 1.0], (n, 4)) * rng.uniform(1, 10, (n, 4)) * 10.0 ** rng.uniform(-8, 11, (n, 4))
    a[: n // 2] = a[: n // 2].astype(np.float32).astype(np.float64)
    return a


def _directed(dtype):
    f = np.dtype(dtype).type
    big = np.nextafter(f(2.0 ** 40), f(0))                     # 2^40 - 1 ulp
    vals = [0.03125, 0.09375, -0.03125, -0.09375, -1e-9, -0.0, 0.0, np.nextafter(f(0), f(1)), big, -big,
            4.5e6 + 0.12345, 4.5e6 + 0.00005, -4.5e6 - 0.99995]
    for c in (9.99995, 99999.99995, 0.99995):
        for t in (np.float32, np.float64):
            m = t(c)
            vals += [m, np.nextafter(m, t(0)), np.nextafter(m, t(1e9)), -m]
    vals = np.array([f(v) for v in vals], dtype=dtype)
    top = 2.0 ** 53 - 1 if dtype == np.float64 else float(np.nextafter(np.float32(2.0 ** 53), np.float32(0)))
    inten = np.array([3.99, -0.5, -3.99, 65535, top, -top, 0.0, -0.0, 0.999], dtype=dtype)
    n = len(vals)
    # every value in every coordinate column
    rows = np.stack([vals, np.roll(vals, 1), np.roll(vals, 2), inten[np.arange(n) % len(inten)]], 1)
    return np.ascontiguousarray(rows, dtype=dtype)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_format_row_counts(n):
    rows = _random_rows(n, 100 + n)
    got, boff = _text(torch.from_numpy(rows).cuda())
    want = _expect(rows)
    assert got == want
    assert boff.tolist() == [0, len(want)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_format_directed_values(dtype):
    rows = _directed(dtype)
    got, _ = _text(torch.from_numpy(rows).cuda())
    assert got == _expect(rows)
    assert b"0.0312 " in got and b"0.0938 " in got and b"-0.0000 " in got and b" 0\n" in got
    if dtype == np.float64:
        assert (b" %d\n" % (2 ** 53 - 1)) in got and b"1099511627775.9999 " in got


def test_format_slices_with_empty_ones():
    rows = _random_rows(257, 7)
    off = np.array([0, 0, 5, 70, 70, 200, 257, 257], dtype=np.int64)
    got, boff = _text(torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda())
    assert boff.shape == (len(off),) and boff[0] == 0 and boff[-1] == len(got)
    for s in range(len(off) - 1):
        assert got[boff[s]:boff[s + 1]] == _expect(rows[off[s]:off[s + 1]]), s
    again, boff2 = _text(rows, off)                       # numpy in, same bytes
    assert again == got and np.array_equal(boff, boff2)


@pytest.fixture(scope="module")
def big():
    rows = _random_rows(100_000, 11)
    return rows, _expect(rows)


def test_format_100k_random_rows(big):
    rows, want = big
    got, _ = _text(torch.from_numpy(rows).cuda())
    assert len(got) == len(want)
    diff = np.count_nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
    assert diff == 0
    got32, _ = _text(torch.from_numpy(rows[:50_000].astype(np.float32)).cuda())      # the float32-exact half
    assert got32 == _expect(rows[:50_000])


def test_format_golden_scene(golden_dir):
    z = R.load_g11(golden_dir)
    pcd = _pcd()
    want = z["file_pcd_bytes"].tobytes()
    hdr = pcd.header_bytes(len(z["file_points"]))
    assert want.startswith(hdr)
    got, _ = _text(torch.from_numpy(np.ascontiguousarray(z["file_points"], dtype=np.float64)).cuda())
    assert got == want[len(hdr):]


OUTSIDE = {"nan": (0, np.nan), "inf": (1, np.inf), "2^41": (2, 2.0 ** 41), "intensity 2^60": (3, 2.0 ** 60)}


@pytest.mark.parametrize("case", list(OUTSIDE))
def test_format_outside_domain_names_the_row(case):
    pcd = _pcd()
    rows = _random_rows(130, 5)
    col, v = OUTSIDE[case]
    rows[70, col] = v
    rows[99, col] = v
    with pytest.raises(pcd.HostFallback, match="row 70") as e:
        pcd.format_rows(torch.from_numpy(rows).cuda())
    assert e.value.row == 70
    rows[70, col] = rows[99, col] = -(2.0 ** 39) if col < 3 else -(2.0 ** 52)
    assert _text(rows)[0] == _expect(rows)


def test_write_pcd_falls_back_to_the_host(tmp_path):
    from pointnet_refine_amd import drive
    pcd = _pcd()
    rows = _random_rows(70, 9)
    rows[33, 0] = np.inf
    a, b = str(tmp_path / "a.pcd"), str(tmp_path / "b.pcd")
    pcd.write_pcd(a, torch.from_numpy(rows).cuda())
    drive.write_scene(b, str(tmp_path / "b.json"), rows, [], "t")
    assert open(a, "rb").read() == open(b, "rb").read()
    with pytest.raises(pcd.HostFallback):
        pcd.write_pcd(a, torch.from_numpy(rows).cuda(), strict=True)
    rows[33, 0] = 1.0
    for v, exc in ((np.nan, ValueError), (np.inf, OverflowError)):
        rows[33, 3] = v
        with pytest.raises(exc) as e:
            pcd.write_pcd(a, torch.from_numpy(rows).cuda())
        assert type(e.value) is exc                      # the host's exception, not HostFallback


# ------------------------------------------------------------------ parser
def _loadtxt(text, ncols):
    if not text.strip():
        return np.zeros((0, ncols), np.float32)
    return np.loadtxt(_io.BytesIO(text), dtype=np.float32).reshape(-1, ncols)


def _check_parse(payload, ncols, text=None):
    got = _pcd().parse_rows(payload, ncols)
    want = _loadtxt(payload if text is None else text, ncols)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    return got


def _table(n, ncols, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (n, ncols)) * 10.0 ** rng.uniform(-4, 7, (n, ncols))
    return b"".join((" ".join(["%.4f"] * (ncols - 1) + ["%d"]) % tuple(r) + "\n").encode() for r in v)


def _fits(line):
    """Every token of the line has an integer of digits <= 2^53: the parser's exact fast path."""
    return all(int(t.replace(b"-", b"").replace(b".", b"")) <= 2 ** 53 for t in line.split())


def test_parse_formatter_texts(big):
    """The formatter's texts back through the strict parser.  '%.4f' of |v| >= 900719925474.0992
    prints 17 digits whose integer exceeds 2^53; the fast path must decline those rows (first one
    named), so the bit comparison runs on the rows it serves and the rest is checked to be declined:
    4 of the directed rows and about 0.04 % of the random ones."""
    pcd = _pcd()
    rows, want = big
    for text in (want, _expect(_directed(np.float64))):
        lines = text.split(b"\n")[:-1]
        ok = [_fits(l) for l in lines]
        assert 0 < ok.count(False) < len(ok) // 2
        _check_parse(b"".join(l + b"\n" for l, k in zip(lines, ok) if k), 4)
        with pytest.raises(pcd.HostFallback) as e:
            pcd.parse_rows(text, 4)
        assert e.value.row == ok.index(False)
    served = rows[np.abs(rows[:, :3]).max(axis=1) < 9.0e11][:4097]
    text, _ = pcd.format_rows(served)
    back = _check_parse(text, 4, text.cpu().numpy().tobytes())             # device text in, no host trip
    assert back.shape[0] == 4097


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
@pytest.mark.parametrize("ncols", [4, 5, 7])
def test_parse_row_and_column_counts(n, ncols):
    _check_parse(_table(n, ncols, 3 * n + ncols), ncols)


def test_parse_line_forms():
    base = _table(300, 4, 2)
    _check_parse(base[:-1], 4)                                             # no final newline
    _check_parse(base.replace(b"\n", b"\r\n"), 4)
    _check_parse(base.replace(b"\n", b"\r\n")[:-1], 4)                    # ends in a bare '\r'
    _check_parse(base.replace(b" ", b"\t"), 4)
    _check_parse(base.replace(b" ", b" \t  ").replace(b"\n", b"  \t\n"), 4)
    _check_parse(b"\n".join(b"  \t" + l + b" " for l in base.split(b"\n")[:-1]), 4)
    toks = b".5 5. +1.5 1e-3\n1E+22 -0.0000 -.5e1 0.\n9007199254740992 1.50000 007 0e0\n+0.0 -0 1e22 1e-22\n"
    got = _check_parse(toks, 4)
    assert np.signbit(got.cpu().numpy()[1, 1]) and np.signbit(got.cpu().numpy()[3, 1])


def _halfway_strings(n, seed):
    """Decimal strings at and on either side of float32 halfway points that the fast path serves:
    h = (2m + 1) * 2^e with a 24-bit m is midway between two float32 neighbours; h itself and h -+ one
    unit in the 16th (else 15th) significant digit, all with an integer of digits <= 2^53."""
    getcontext().prec = 60
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < 3 * n:
        m = int(rng.integers(2 ** 23, 2 ** 24))
        e = int(rng.integers(-8, 22))
        h = Fraction(2 * m + 1) * Fraction(2) ** e
        hd = Decimal(h.numerator) / Decimal(h.denominator)                 # exact: a dyadic rational
        for digits in (16, 15):
            q = Decimal(1).scaleb(hd.adjusted() - (digits - 1))
            trio = [hd - q, hd, hd + q]
            if all(int("".join(map(str, t.as_tuple().digits))) <= 2 ** 53 for t in trio):
                break
        sign = "-" if rng.random() < 0.5 else ""
        out += [sign + format(t, "f") for t in trio]
    return out


def test_parse_exact_halfway_decimals_and_their_neighbours():
    strs = _halfway_strings(10_000, 4)                   # 20,000 off the halfway point + the 10,000 ties
    assert len(strs) == 30_000 and max(len(s.replace("-", "").replace(".", "").lstrip("0")) for s in strs) <= 17
    text = "".join(" ".join(strs[i:i + 4]) + "\n" for i in range(0, len(strs), 4)).encode()
    got = _check_parse(text, 4).cpu().numpy().reshape(-1)
    twice = np.array([float(s) for s in strs]).astype(np.float32)         # decimal -> double -> float32
    assert np.array_equal(got.view(np.int32), twice.view(np.int32))
    lo, hi = got[0::3], got[2::3]
    assert np.all(lo != hi)                                                 # the two sides round apart


def _double_rounding_strings(n, seed):
    """2n fast-path decimals that hug float32 halfway points closer than a double can tell.
    h = (2j + 1) * 2^e with a 24-bit j and e in [-60, -30) lies midway between the float32 values
    j * 2^(e+1) and (j + 1) * 2^(e+1) and has far more than 17 decimal digits; with the largest k <= 22
    that keeps h * 10^k <= 2^53, m = floor(h * 10^k) and m + 1 give the nearest served decimals below
    and above it (written m e-k or as a plain fraction).  Returns the strings and the DIRECT correctly
    rounded float32 of each: the lower neighbour for the one below h, the upper for the one above."""
    rng = np.random.default_rng(seed)
    strs, direct = [], []
    while len(strs) < 2 * n:
        j, e = int(rng.integers(2 ** 23, 2 ** 24)), int(rng.integers(-60, -30))
        h = Fraction(2 * j + 1) * Fraction(2) ** e
        k = 22
        while h * 10 ** k > 2 ** 53:
            k -= 1
        m = (h * 10 ** k).__floor__()
        assert Fraction(m, 10 ** k) < h < Fraction(m + 1, 10 ** k) and m + 1 <= 2 ** 53
        sign = "-" if rng.random() < 0.5 else ""
        for mm, nb in ((m, j), (m + 1, j + 1)):
            d = str(mm)
            if (len(strs) // 2) % 2:
                tok = f"{d}e-{k}"
            else:
                tok = "0." + d.rjust(k, "0") if k >= len(d) else d[:-k] + "." + d[-k:]
            strs.append(sign + tok)
            direct.append(float(Fraction(nb) * Fraction(2) ** (e + 1)) * (-1.0 if sign else 1.0))
    return strs, np.array(direct, dtype=np.float64).astype(np.float32)          # exact: float32 values


def test_parse_rounds_through_a_double_not_directly():
    """np.loadtxt rounds decimal -> double -> float32.  When a string lies within half a double ulp of
    a float32 halfway point its double IS the tie, and the cast then goes to the even neighbour, which
    for about half of those strings is not the float32 nearest to the decimal.  The served decimals
    are 1/m apart (relative 1.1e-16 .. 1e-15), half a double ulp is 5.5e-17 .. 1.1e-16 relative, so
    several per cent of the strings must differ from direct rounding; 2.5 % is asked.  A parser that
    converted decimal -> float32 directly would equal `direct` everywhere and fail the bit comparison."""
    strs, direct = _double_rounding_strings(10_000, 4)
    assert len(strs) == 20_000
    text = "".join(" ".join(strs[i:i + 4]) + "\n" for i in range(0, len(strs), 4)).encode()
    got = _check_parse(text, 4).cpu().numpy().reshape(-1)                        # == np.loadtxt, bit for bit
    differ = int(np.count_nonzero(got.view(np.int32) != direct.view(np.int32)))
    print(f"double rounding changes {differ} of {len(strs)} strings")
    assert differ >= 500
    twice = np.array([float(s) for s in strs]).astype(np.float32)
    assert np.array_equal(got.view(np.int32), twice.view(np.int32))
    one = _pcd().parse_rows(b"4839814891965943e-21\n", 1).cpu().numpy()
    assert one[0, 0] == np.float32(4.839815e-06) and one[0, 0] != np.float32(4.8398147e-06)


@pytest.mark.parametrize("length", [4095, 4096, 4097, 8191, 8193, 15, 17])
def test_parse_lengths_around_the_chunk(length):
    head, rows = b"1 2 3 4\n", _table(400, 4, 6).split(b"\n")[:-1]
    cut = b""
    for r in rows:
        if len(head) + len(cut) + len(r) + 1 > length:
            break
        cut += r + b"\n"
    text = b" " * (length - len(head) - len(cut)) + head + cut           # leading blanks make up the length
    assert len(text) == length
    _check_parse(text, 4)


@pytest.mark.parametrize("shift", [1, 3, 8, 15])
def test_parse_unaligned_payload(shift):
    text = _table(700, 4, 8)
    whole = torch.from_numpy(np.frombuffer(b"\n" * shift + text + b"\n9 9\n", dtype=np.uint8).copy()).cuda()
    payload = whole[shift:shift + len(text)]
    assert payload.data_ptr() % 16 == shift
    _check_parse(payload, 4, text)


DECLINED = {
    "25 digits": b"1234567890123456789012345 2 3 4",
    "1e23": b"1 1e23 3 4",
    "nan": b"1 2 nan 4",
    "blank line": b"",
    "comment": b"# 1 2 3 4",
    "comma": b"1,2 3 4 5",
    "short row": b"1 2 3",
}


def _with_row(line, at=70, n=130):
    rows = _table(n, 4, 10).split(b"\n")[:-1]
    rows[at] = line
    return b"\n".join(rows) + b"\n"


@pytest.mark.parametrize("case", list(DECLINED))
def test_parse_declines_and_names_the_row(case):
    pcd = _pcd()
    with pytest.raises(pcd.HostFallback, match="row 70") as e:
        pcd.parse_rows(_with_row(DECLINED[case]), 4)
    assert e.value.row == 70


@pytest.mark.parametrize("case", list(DECLINED))
def test_read_pcd_falls_back_like_the_host(case, tmp_path, capsys):
    from pointnet_refine_amd import io
    pcd = _pcd()
    path = str(tmp_path / "s.pcd")
    with open(path, "wb") as f:
        f.write(pcd.header_bytes(130) + _with_row(DECLINED[case]))
    want = io.load_pcd_data(path)
    got = pcd.read_pcd(path)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))
    if case in ("comma", "short row"):
        assert want.shape == (0, 4)
    else:
        assert len(want) >= 129
    with pytest.raises(pcd.HostFallback):
        pcd.read_pcd(path, strict=True)


# ------------------------------------------------------------------ unpack and end to end
@pytest.mark.parametrize("n", [0, 1, 65, 4097])
@pytest.mark.parametrize("record", [14, 16])
def test_read_binary_records(n, record, tmp_path):
    from pointnet_refine_amd import io
    pcd = _pcd()
    rng = np.random.default_rng(n + record)
    xyz = (rng.uniform(-1, 1, (n, 3)) * 10.0 ** rng.uniform(-3, 6, (n, 3))).astype("<f4")
    if record == 14:
        rec = np.zeros(n, dtype=io._XYZ_F32_I_U2)
        rec["intensity"] = rng.integers(0, 65536, n)
    else:
        rec = np.zeros(n, dtype=io._XYZI_F32)
        rec["intensity"] = rng.uniform(0, 255, n)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    path = str(tmp_path / "m.pcd")
    with open(path, "wb") as f:
        f.write(f"VERSION 0.7\nFIELDS x y z intensity\nWIDTH {n}\nHEIGHT 1\nPOINTS {n}\nDATA binary\n".encode())
        f.write(rec.tobytes())
    want = io.load_pcd_data(path)
    got = pcd.read_pcd(path, strict=True)
    assert tuple(got.shape) == want.shape == (n, 4) and got.is_cuda
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    if record == 14 and n > 1:                            # the kernel at an unaligned payload
        raw = torch.from_numpy(np.frombuffer(b"\x07" * 3 + rec.tobytes(), dtype=np.uint8).copy()).cuda()
        again = pcd.unpack_records14(raw[3:], n)
        assert np.array_equal(again.cpu().numpy().view(np.int32), want.view(np.int32))


def test_read_pcd_missing_and_mismatched(tmp_path, capsys):
    pcd = _pcd()
    got = pcd.read_pcd(str(tmp_path / "nope.pcd"))
    assert tuple(got.shape) == (0, 4) and got.is_cuda
    path = str(tmp_path / "bad.pcd")
    with open(path, "wb") as f:
        f.write(b"POINTS 3\nDATA binary\n" + b"\x00" * 40)
    assert tuple(pcd.read_pcd(path).shape) == (0, 4)
    assert "returning an empty cloud" in capsys.readouterr().out


def test_write_pcds_matches_write_scene(tmp_path):
    import test_drive_gpu as TG
    from pointnet_refine_amd import drive, io
    pcd = _pcd()
    cloud, poses = TG._synthetic_drive(30_000, 3, seed=5)
    points, offsets, _ = drive.slice_cloud(cloud, poses)
    off = offsets.cpu().numpy()
    assert len(off) == 4 and np.all(np.diff(off) > 0)
    paths = [str(tmp_path / f"d{s}.pcd") for s in range(3)]
    pcd.write_pcds(paths, points, offsets, strict=True)
    host = points.cpu().numpy()
    for s, p in enumerate(paths):
        ref = str(tmp_path / f"h{s}.pcd")
        drive.write_scene(ref, str(tmp_path / "h.json"), host[off[s]:off[s + 1]], [], "t")
        assert open(p, "rb").read() == open(ref, "rb").read()
        want = io.load_pcd_data(ref)
        got = pcd.read_pcd(p, strict=True)
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    pcd.write_pcds([None, paths[1], None], points, offsets, strict=True)       # None: not written
    pcd.write_pcd(paths[0], points[off[1]:off[2]], strict=True)
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read()


def test_slice_drive_files_equal_write_scene(tmp_path):
    import test_drive_gpu as TG
    from pointnet_refine_amd import drive
    drive_dir, out_dir = str(tmp_path / "drive"), str(tmp_path / "scenes")
    os.makedirs(drive_dir)
    gt, _, _ = TG._write_drive(drive_dir)
    res = drive.slice_drive(drive_dir, gt, out_dir, verbose=False)
    assert len(res["written"]) >= 3
    off, host = res["offsets"].cpu().numpy(), res["points"].cpu().numpy()
    for name in res["written"]:
        s = res["names"].index(name)
        ref = str(tmp_path / "ref.pcd")
        drive.write_scene(ref, str(tmp_path / "ref.json"), host[off[s]:off[s + 1]], res["items"][s], name)
        assert open(os.path.join(out_dir, name + ".pcd"), "rb").read() == open(ref, "rb").read()
        assert open(os.path.join(out_dir, name + ".json"), "rb").read() == open(str(tmp_path / "ref.json"), "rb").read()
    assert sorted(os.listdir(out_dir)) == sorted(f"{n}{ext}" for n in res["written"] for ext in (".json", ".pcd"))


def test_predictions_to_scenes_files_equal_write_prediction_scene(golden_dir, tmp_path):
    import json
    import test_predictions_cpu as RP
    from pointnet_refine_amd import predictions
    z = RP.load_g12(golden_dir)
    drive_dir, gt, results = RP._write_drive(z, str(tmp_path / "drive"))
    out_dir = str(tmp_path / "scenes")
    res = predictions.predictions_to_scenes(drive_dir, gt, results, out_dir, verbose=False)
    assert len(res["written"]) >= 1
    off, host = res["offsets"].cpu().numpy(), res["points"].cpu().numpy()
    rp, rj = str(tmp_path / "ref.pcd"), str(tmp_path / "ref.json")
    for ts in res["written"]:
        n = res["frames"].index(ts)
        s = res["slice"][n]
        predictions.write_prediction_scene(rp, rj, host[off[s]:off[s + 1]], res["items"][n], res["pose_ts"][n], ts)
        assert open(os.path.join(out_dir, f"{ts}.pcd"), "rb").read() == open(rp, "rb").read()
        assert open(os.path.join(out_dir, f"{ts}.json"), "rb").read() == open(rj, "rb").read()
        assert json.load(open(rj))["result_timestamp"] == str(ts)


def test_arguments_are_checked_before_a_kernel_runs():
    pcd = _pcd()
    rows = _random_rows(100, 21)
    dev_rows = torch.from_numpy(rows).cuda()
    for off in ([0, 60, 40, 100], [0, 101], [-1, 100]):
        with pytest.raises(ValueError, match="offsets"):
            pcd.format_rows(dev_rows, np.array(off, dtype=np.int64))
    flat = torch.zeros(4 * 100 + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(rows.astype(np.float32).reshape(-1)).cuda()
    shifted = flat[1:].view(100, 4)                        # rows 4 bytes off the 16-byte grid
    assert shifted.data_ptr() % 16 == 4
    assert _text(shifted)[0] == _expect(rows.astype(np.float32))
    pay = torch.zeros(14 * 10, dtype=torch.uint8, device="cuda")
    assert tuple(pcd.unpack_records14(pay, 10).shape) == (10, 4)
    with pytest.raises(ValueError, match="140 bytes"):
        pcd.unpack_records14(pay[:-1], 10)
    with pytest.raises(ValueError):
        pcd.unpack_records14(pay.view(torch.int16), 10)
    with pytest.raises(RuntimeError, match="CUDA"):
        pcd.unpack_records14(pay.cpu(), 10)
