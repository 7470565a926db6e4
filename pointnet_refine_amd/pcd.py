"""PCD codec: the reference's scene files (save_pcd, tools/generate_train_data.py:184-190;
load_pcd_data, src/dataset.py:31-76) formatted and parsed on the GPU (``csrc/prh_pcd.hpp``), so a
cloud that is already on the device meets the disk as one byte copy.

  format_rows     HIP: (T,4) rows -> the text '%.4f %.4f %.4f %d\\n' of every row, byte for byte what
                  Python's % operator (np.savetxt) writes, with the byte span of every slice
  parse_rows      HIP: the payload of an ASCII PCD -> (P, ncols) float32 with np.loadtxt's bits
  write_pcds / write_pcd   the ten header lines + one slice of that text per file
  write_pcd_host  the same file from np.savetxt: the package's one host writer and header text
  read_pcd        io.load_pcd_data's result as a CUDA tensor: ASCII through parse_rows, 14-byte
                  binary records through an unpack kernel, 16-byte records as a view

The device paths are strict: a row they cannot serve exactly (a value outside the formatter's
domain - finite |x|,|y|,|z| < 2^40, finite |intensity| < 2^53; a token outside the parser's exact
fast path, a blank or comment line, a ragged row) raises HostFallback naming the row, and
write_pcd(s) / read_pcd(strict=False) then redo that call through the host functions
(write_pcd_host, the np.savetxt writer drive.write_scene is built on; io.load_pcd_data), so bytes, values and exceptions are the
host's.  format_rows, parse_rows and read_pcd have no CPU fallback: without a GPU they raise
RuntimeError.
"""
import numpy as np
import torch

from . import _gpu as G
from . import _lib as L

FIELDS = ("x", "y", "z", "intensity")


class HostFallback(ValueError):
    """The device codec declined a row (``.row``); the host path serves the call."""

    def __init__(self, what, row):
        super().__init__(f"{what}: row {row} is outside the device path")
        self.row = int(row)


# ------------------------------------------------------------------ host side: the header
def header_bytes(n):
    """The ten header lines of the reference's scene files for n points (the package's one copy)."""
    return (f"VERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
            f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA ascii\n").encode()


def parse_header(buf):
    """The header of a PCD file held in buf (bytes-like), read as io.load_pcd_data reads it: lines up
    to and including the one that starts with DATA.  Returns {'length' (bytes, the payload starts
    there), 'lines' (count), 'data' (b'ascii', b'binary', ...), 'points' (int or None), 'fields'
    (list of bytes)}; raises ValueError without a DATA line."""
    pos, lines, info = 0, 0, {"points": None, "fields": []}
    while True:
        end = buf.find(b"\n", pos)
        raw = bytes(buf[pos:len(buf) if end < 0 else end + 1])
        if not raw:
            raise ValueError("no DATA line in the PCD header")
        pos += len(raw)
        lines += 1
        line = raw.strip()
        if line.startswith(b"POINTS") and info["points"] is None:
            info["points"] = int(line.split()[1])
        elif line.startswith(b"FIELDS"):
            info["fields"] = line.split()[1:]
        elif line.startswith(b"DATA"):
            info.update(length=pos, lines=lines, data=line.split()[1])
            return info


def write_pcd_host(path, points):
    """The reference's save_pcd on the host, byte for byte: the header and np.savetxt's '%.4f %.4f
    %.4f %d' rows (intensity truncated as int() does).  points: (n,4) rows, numpy or tensor.  The
    .pcd half of drive.write_scene and predictions.write_prediction_scene, and what write_pcds
    falls back to."""
    rows = np.asarray(torch.as_tensor(points).cpu() if torch.is_tensor(points) else points, dtype=np.float64)
    rows = rows.reshape(-1, 4)
    with open(path, "w") as f:
        f.write(header_bytes(len(rows)).decode())
        if len(rows):
            np.savetxt(f, rows, fmt="%.4f %.4f %.4f %d", newline="\n")


# ------------------------------------------------------------------ GPU side
def _rows_t(points, what):
    pts = G.as_cuda(points, G.device("pcd"), what)
    if pts.dtype not in (torch.float64, torch.float32):
        pts = pts.to(torch.float64)
    if pts.dim() != 2 or pts.shape[1] != 4:
        raise ValueError(f"{what}: points must be (T,4), got {tuple(pts.shape)}")
    pts = pts.contiguous()
    return pts if pts.data_ptr() % 16 == 0 else pts.clone()       # the kernels load whole rows: 16-byte aligned


def format_rows(points, offsets=None):
    """The text of points (T,4) fp64 or fp32, numpy or CUDA tensor: '%.4f %.4f %.4f %d\\n' per row.
    offsets (S+1,) int64 rows of each slice, as slice_cloud returns them (None: one slice).  Returns
    (text (bytes,) uint8 CUDA, byte_offsets (S+1,) int64 CUDA): slice s is
    text[byte_offsets[s]:byte_offsets[s+1]].  Raises HostFallback for the first row outside the
    domain (module docstring).  Bitwise reproducible."""
    pts = _rows_t(points, "format_rows")
    dev = pts.device
    n = pts.shape[0]
    off = None
    if offsets is not None:
        off = torch.as_tensor(offsets).to(dev, torch.int64).contiguous()
        if off.dim() != 1 or off.numel() < 1:
            raise ValueError("format_rows: offsets must be (S+1,)")
        lo, hi, ascending = torch.stack((off[0], off[-1], (off[1:] >= off[:-1]).all().to(torch.int64))).tolist()
        if not (ascending and lo >= 0 and hi <= n):
            raise ValueError(f"format_rows: offsets must ascend within [0, {n}]")
    n_s = 1 if off is None else off.numel() - 1
    lib = L.lib()
    group = lib.prh_pcd_group_rows()
    n_g = -(-n // group)
    row_bytes = torch.empty((n,), dtype=torch.uint8, device=dev)
    group_bytes = torch.empty((n_g,), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int64, device=dev)
    nb = lib.prh_pcd_format_workspace_bytes(n)
    ws = G.workspace(nb, dev)
    is64 = 1 if pts.dtype == torch.float64 else 0
    L.check(lib.prh_pcd_format_count(G.ptr(pts), is64, n, G.ptr(row_bytes), G.ptr(group_bytes), G.ptr(status), G.ptr(ws),
                                     nb, dev.index, G.stream(dev)), "prh_pcd_format_count")
    group_off = G.exclusive_scan(group_bytes)
    bad, total = torch.stack((status[0], group_off[-1])).tolist()
    if bad >= 0:
        raise HostFallback("format_rows", bad)
    text = torch.empty((total,), dtype=torch.uint8, device=dev)
    byte_off = torch.empty((n_s + 1,), dtype=torch.int64, device=dev)
    L.check(lib.prh_pcd_format_write(G.ptr(pts), is64, n, G.ptr(row_bytes), G.ptr(group_off), G.ptr(off), n_s, G.ptr(text),
                                     total, G.ptr(byte_off), dev.index, G.stream(dev)), "prh_pcd_format_write")
    return text, byte_off


def parse_rows(payload, ncols):
    """The rows of an ASCII PCD payload (uint8 CUDA tensor of any alignment, or bytes) as (P, ncols)
    float32 CUDA with the bits np.loadtxt(dtype=np.float32) returns.  Fields are separated by runs
    of blanks or tabs; '\\r\\n' and a missing final newline are accepted.  Raises HostFallback for
    the first row outside the exact fast path (module docstring)."""
    if torch.is_tensor(payload):
        if not payload.is_cuda:
            raise RuntimeError("parse_rows: tensors must be CUDA tensors (there is no CPU fallback)")
        G.device("pcd")
        if payload.dtype != torch.uint8 or payload.dim() != 1:
            raise ValueError("parse_rows: payload must be a 1-D uint8 tensor")
        pay = payload.detach().contiguous()
    else:
        dev = G.device("pcd")
        pay = (torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(dev) if len(payload)
               else torch.empty((0,), dtype=torch.uint8, device=dev))
    ncols = int(ncols)
    if ncols < 1:
        raise ValueError("parse_rows: ncols must be at least 1")
    dev = pay.device
    n = pay.numel()
    if n == 0:
        return torch.empty((0, ncols), dtype=torch.float32, device=dev)
    lib = L.lib()
    n_b = lib.prh_pcd_index_blocks(G.ptr(pay), n)
    block_lines = torch.empty((n_b,), dtype=torch.int32, device=dev)
    L.check(lib.prh_pcd_index_count(G.ptr(pay), n, G.ptr(block_lines), dev.index, G.stream(dev)), "prh_pcd_index_count")
    block_off = G.exclusive_scan(block_lines)
    lines, last = torch.stack((block_off[-1], pay[-1].to(torch.int64))).tolist()
    rows = lines + (0 if last == 10 else 1)
    row_start = torch.empty((rows + 1,), dtype=torch.int64, device=dev)
    L.check(lib.prh_pcd_index_write(G.ptr(pay), n, G.ptr(block_off), G.ptr(row_start), rows, dev.index, G.stream(dev)),
            "prh_pcd_index_write")
    out = torch.empty((rows, ncols), dtype=torch.float32, device=dev)
    status = torch.empty((1,), dtype=torch.int64, device=dev)
    nb = lib.prh_pcd_parse_workspace_bytes(rows)
    ws = G.workspace(nb, dev)
    L.check(lib.prh_pcd_parse(G.ptr(pay), n, G.ptr(row_start), rows, ncols, G.ptr(out), G.ptr(status), G.ptr(ws), nb,
                              dev.index, G.stream(dev)), "prh_pcd_parse")
    bad = int(status.item())
    if bad >= 0:
        raise HostFallback("parse_rows", bad)
    return out


def unpack_records14(payload, n_points):
    """n_points 14-byte records (xyz float32 + uint16 intensity) in a uint8 CUDA tensor -> (P,4) float32."""
    if not torch.is_tensor(payload) or not payload.is_cuda:
        raise RuntimeError("unpack_records14: payload must be a CUDA tensor (there is no CPU fallback)")
    n_points = int(n_points)
    if payload.dtype != torch.uint8 or payload.dim() != 1 or n_points < 0 or payload.numel() < 14 * n_points:
        raise ValueError(f"unpack_records14: payload must be 1-D uint8 with at least {14 * n_points} bytes")
    payload = payload.detach().contiguous()
    dev = payload.device
    out = torch.empty((n_points, 4), dtype=torch.float32, device=dev)
    L.check(L.lib().prh_pcd_unpack14(G.ptr(payload), n_points, G.ptr(out), dev.index, G.stream(dev)), "prh_pcd_unpack14")
    return out


def write_pcds(paths, points, offsets, strict=False):
    """One ASCII PCD per slice of points (T,4) / offsets (S+1,), the files drive.write_scene writes:
    the text comes from format_rows, crosses to the host in one copy and every file gets one write.
    paths: S entries, None = that slice is not written.  A row outside the device domain redoes the
    call on the host (np.savetxt: its bytes, its ValueError / OverflowError) unless strict, which
    lets HostFallback through."""
    off = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)
    if len(paths) != len(off) - 1:
        raise ValueError(f"write_pcds: {len(paths)} paths for {len(off) - 1} slices")
    try:
        text, byte_off = format_rows(points, off)
    except HostFallback:
        if strict:
            raise
        host = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
        for s, path in enumerate(paths):
            if path is not None:
                write_pcd_host(path, host[off[s]:off[s + 1]])
        return
    text, boff = memoryview(text.cpu().numpy()), byte_off.cpu().numpy()
    for s, path in enumerate(paths):
        if path is not None:
            with open(path, "wb") as f:
                f.write(b"".join((header_bytes(int(off[s + 1] - off[s])), text[boff[s]:boff[s + 1]])))


def write_pcd(path, points, strict=False):
    """write_pcds for one file holding every row of points."""
    n = len(points)
    write_pcds([path], points, np.array([0, n], dtype=np.int64), strict=strict)


def _upload(arr, dev):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def read_pcd(path, device=None, strict=False):
    """io.load_pcd_data(path) as a (P, C) float32 CUDA tensor, bit for bit (a one-row ASCII file gives
    (1, C); an ASCII file without rows gives (0, C) with C from FIELDS, else 4).  The header is read
    on the host; an ASCII payload goes through parse_rows with C taken from its first line, 14-byte
    binary records through the unpack kernel, 16-byte records are a view of the upload.  Anything
    else - another layout, a file the device parser declines (unless strict: HostFallback) - goes
    through io.load_pcd_data, which never raises: a missing file, a bad header or a ragged file
    give an empty (0,4) tensor and its printed message."""
    from .io import load_pcd_data
    dev = G.device("pcd", device)

    def host():
        arr = load_pcd_data(path)
        return _upload(np.atleast_2d(arr) if arr.size else arr.reshape(0, arr.shape[-1] if arr.ndim == 2 else 4), dev)

    try:
        with open(path, "rb") as f:
            buf = bytearray(f.read())
        hdr = parse_header(buf)
        n_pay = len(buf) - hdr["length"]
        kind = hdr["data"]
        if kind != b"ascii" and hdr["points"] is None:
            raise ValueError("no POINTS line")
    except Exception:
        return host()                                   # load_pcd_data prints the reason
    pay = (torch.frombuffer(buf, dtype=torch.uint8, offset=hdr["length"], count=n_pay).to(dev) if n_pay
           else torch.empty((0,), dtype=torch.uint8, device=dev))
    if kind == b"ascii":
        if n_pay == 0:
            return torch.empty((0, len(hdr["fields"]) or 4), dtype=torch.float32, device=dev)
        end = buf.find(b"\n", hdr["length"])
        ncols = len(bytes(buf[hdr["length"]:len(buf) if end < 0 else end]).split()) or 4
        try:
            return parse_rows(pay, ncols)
        except HostFallback:
            if strict:
                raise
            return host()
    n = hdr["points"]
    if n >= 0 and n_pay == n * 16:
        return pay.view(torch.float32).view(n, 4)
    if n >= 0 and n_pay == n * 14:
        return unpack_records14(pay, n)
    return host()
