"""What the tool modules (drive, predictions, bev, pcd, metrics, context, fuse, link, view3d, support, ground, align)
share on their way to the library: the device getter, pointers and streams for ctypes, the throwaway workspace, the
exclusive scan between a count and a write call, the upload rule (numpy is uploaded, a CUDA tensor is used where it
is, a CPU tensor is refused), the two-pass polyline clip that drive.clip_lines and predictions.clip_lines_frames both
are, and what ground and align take a sliced cloud with: host copies, checked offsets, the (T,4) points and the
per-slice cell grids.  ops / model / train_step do not use this module: their workspace is a grow-only cache per
stream and their pointers treat empty tensors differently.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

_NUMPY = {None: None, torch.float32: np.float32, torch.float64: np.float64}


def device(module, device=None):
    """The CUDA device a tool module runs on (device, or the current one); RuntimeError without one."""
    dev = torch.device("cuda" if device is None or not torch.cuda.is_available() else device)
    if not torch.cuda.is_available() or dev.type != "cuda":
        raise RuntimeError(f"pointnet_refine_amd.{module} needs a GPU (there is no CPU fallback)")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def workspace(nbytes, dev):
    """A scratch buffer for one library call: never empty, never reused."""
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=dev)


def exclusive_scan(counts):
    """(n+1,) int64: 0 followed by the running sums of counts (n,), on counts' device."""
    out = torch.zeros((counts.numel() + 1,), dtype=torch.int64, device=counts.device)
    if counts.numel():
        out[1:] = torch.cumsum(counts, 0)
    return out


def csr_offsets(counts):
    """(n+1,) int64 on the host: 0 followed by the running sums of counts, an array or a list of
    ints; an empty one gives [0]."""
    out = np.zeros(len(counts) + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.asarray(counts, dtype=np.int64))
    return out


def as_cuda(x, dev, what, dtype=None):
    """x as a contiguous CUDA tensor of dtype (None: its own): a numpy array (or nested list) is
    converted on the host and uploaded to dev, a CUDA tensor stays on its device, a CPU tensor raises."""
    if torch.is_tensor(x):
        if not x.is_cuda:
            raise RuntimeError(f"{what}: tensors must be CUDA tensors (there is no CPU fallback)")
        t = x.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=_NUMPY[dtype])).to(dev)
    return (t if dtype is None else t.to(dtype)).contiguous()


def host(x, dtype):
    """x (a tensor anywhere, or anything numpy takes) as a numpy array of dtype."""
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(dtype, copy=False)


def offsets(x, n, what, name):
    """x as (S+1,) int64 on the host; ValueError unless it rises from 0 to n."""
    off = host(x, np.int64).reshape(-1)
    if len(off) < 1 or off[0] != 0 or off[-1] != n or np.any(np.diff(off) < 0):
        raise ValueError(f"{what}: {name} must rise from 0 to {n}")
    return off


def points4(points, dev, what):
    """(T,4) float64 or float32 CUDA, aligned to two coordinates: numpy is uploaded once, a CUDA
    tensor stays where it is."""
    shape = tuple(points.shape) if torch.is_tensor(points) else np.shape(points)
    if len(shape) != 2 or shape[1] != 4:
        raise ValueError(f"{what}: points must be (T,4) x y z intensity, got {shape}")
    if not torch.is_tensor(points):
        points = np.asarray(points)
        if points.dtype not in (np.float32, np.float64):
            raise ValueError(f"{what}: points must be float64 or float32, got {points.dtype}")
    elif points.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: points must be float64 or float32, got {points.dtype}")
    t = as_cuda(points, dev, what)
    return t.clone() if t.numel() and t.data_ptr() % 16 else t


def box_grids(xy, off, reach, cell, max_cells):
    """Per slice a uniform xy grid, cell metres wide, over the box of its rows of xy (N,2) float64 (off (S+1,) int64)
    expanded by reach (a scalar, or (S,)): nx = floor((hi - lo) / cell) + 1.  cell is doubled until all grids together
    have at most max_cells cells.  Returns {'origin' (S,2) float64, 'shape' (S,2) int32 = nx ny (0 0 for a slice
    without a row), 'cell_base' (S,) int64, 'n_cells', 'cell'}."""
    n_s, cell = len(off) - 1, float(cell)
    origin = np.zeros((n_s, 2))
    shape = np.zeros((n_s, 2), dtype=np.int64)
    used = np.flatnonzero(np.diff(off) > 0)
    if len(used):
        start = off[:-1][used]
        r = np.broadcast_to(np.asarray(reach, dtype=np.float64), (n_s,))[used, None]
        lo = np.stack([np.minimum.reduceat(xy[:, c], start) for c in (0, 1)], 1) - r
        hi = np.stack([np.maximum.reduceat(xy[:, c], start) for c in (0, 1)], 1) + r
        origin[used] = lo
        while True:
            n = np.floor((hi - lo) / cell).astype(np.int64) + 1
            if int((n[:, 0] * n[:, 1]).sum()) <= max_cells:
                break
            cell *= 2.0
        shape[used] = n
    base = np.zeros(n_s, dtype=np.int64)
    cells = shape[:, 0] * shape[:, 1]
    if n_s:
        base[1:] = np.cumsum(cells)[:-1]
    return {"origin": origin, "shape": shape.astype(np.int32), "cell_base": base, "n_cells": int(cells.sum()), "cell": cell}


def poses(poses_xyzq, dev, what):
    """(S,7) float64 CUDA x y z qx qy qz qw."""
    if not torch.is_tensor(poses_xyzq):
        poses_xyzq = np.asarray(poses_xyzq, dtype=np.float64).reshape(-1, 7)
    return as_cuda(poses_xyzq, dev, what, torch.float64).reshape(-1, 7)


def lines_csr(lines, dev):
    """A list of (n,3) polylines (None: no vertex) as CSR: (vertices (V,3) float64 CUDA, offsets
    (L+1,) int64 CUDA, the same offsets as numpy)."""
    arrs = [np.zeros((0, 3)) if l is None else np.asarray(l, dtype=np.float64).reshape(-1, 3) for l in lines]
    off = csr_offsets([len(a) for a in arrs])
    verts = np.concatenate(arrs) if off[-1] > 0 else np.zeros((0, 3))
    return torch.from_numpy(np.ascontiguousarray(verts)).to(dev), torch.from_numpy(off).to(dev), off


def clip_two_pass(names, lines, ps, segment_len, return_counts):
    """Count, scan, write for every (pose, line) pair.  names: the library's workspace-size, count
    and write functions of one clip rule; ps: poses() on the device to run on.  Returns, per pose,
    the list of (line index, (k,3) float64 numpy) with k > 1, in line order; return_counts=True also
    returns the (n_poses, n_lines) int array of vertex counts before that rule."""
    lib = L.lib()
    ws_bytes, count, write = (getattr(lib, n) for n in names)
    dev = ps.device
    n_p, n_l = ps.shape[0], len(lines)
    verts, off_t, _ = lines_csr(lines, dev)
    counts = torch.zeros((n_p * n_l,), dtype=torch.int32, device=dev)
    nb = ws_bytes(n_p)
    ws = workspace(nb, dev)
    L.check(count(ptr(verts), ptr(off_t), n_l, ptr(ps), n_p, float(segment_len), ptr(counts), ptr(ws), nb, dev.index,
                  stream(dev)), names[1])
    out_off = exclusive_scan(counts)
    total = int(out_off[-1].item())
    out = torch.empty((total, 3), dtype=torch.float64, device=dev)
    if total:
        L.check(write(ptr(verts), ptr(off_t), n_l, ptr(ps), n_p, float(segment_len), ptr(out_off), ptr(out), ptr(ws), nb,
                      dev.index, stream(dev)), names[2])
    out, oo = out.cpu().numpy(), out_off.cpu().numpy()
    cnt = np.diff(oo).reshape(n_p, n_l)
    per_pose = [[(l, out[oo[p * n_l + l]:oo[p * n_l + l + 1]].copy()) for l in range(n_l) if cnt[p, l] > 1]
                for p in range(n_p)]
    return (per_pose, cnt) if return_counts else per_pose
