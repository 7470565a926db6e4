"""Drive slicer: the reference's data preparation (tools/generate_train_data.py,
tools/augment_train_data.py) - one merged cloud, a pose per frame and one GT-polyline JSON in,
ego-frame 50 m scenes out, the files ``io.load_pcd_data`` / ``load_scene_items`` /
``SceneSampleStream`` read.  The reference makes a full numpy pass over the whole cloud for every
slice; here every slice of a drive comes out of two HIP passes over the cloud
(``csrc/prh_drive.hpp``).

  load_poses / plan_slices   host: the pose JSONs and the 25 m walk along x (:16-51,229-245,280)
  slice_cloud                HIP: float32 60 m radius test + fp64 ego transform + |x| <= 25 crop
                             for all slices at once, points in cloud order (:247-261)
  clip_lines                 HIP: every GT polyline transformed and clipped per slice (:145-182,263-273)
  apply_noise                HIP: the deterministic half of generate_noisy_line (augment :18-54)
  noisy_candidates           HIP: the same with the draws from a counter hash, fresh per seed
  write_scene / slice_drive  host: the reference's two files (:184-209: pcd.write_pcd_host + this
                             module's JSON) and the whole pipeline (slice_drive's .pcd text is
                             formatted on the device: pcd.write_pcds)

    res = slice_drive("DRIVE_annotation_raw_data", "DRIVE.bag.json", "train_data")
    stream = SceneSampleStream("train_data", augment=(0.1, 0.25, 0.4), batch_size=32)

slice_cloud, clip_lines, apply_noise and noisy_candidates have no CPU fallback: without a GPU they
raise RuntimeError.  The plumbing to the library (device, pointers, uploads, the count / scan /
write clip driver shared with predictions.clip_lines_frames) is in _gpu.py.
"""
import ctypes as C
import glob
import json
import os

import numpy as np
import torch

from . import _gpu as G
from . import _lib as L
from .pcd import write_pcd_host, write_pcds

SEGMENT_LEN = 50.0           # generate_train_data.py:11-12
STRIDE = 25.0
RADIUS = 60.0                # :252 (dx**2 + dy**2 < 3600)
MAX_POSE_GAP = 10.0          # :241
NOISE_SCALES = (0.1, 0.25, 0.4)     # augment_train_data.py:71-75
MAX_SCALES = 8


# ------------------------------------------------------------------ host side
def load_poses(pose_dir):
    """The pose JSONs of a drive (:16-51): list of {'ts', 'filename_ts', 'x', 'y', 'z', 'q': [qx,qy,qz,qw]}
    sorted by file name; a file that cannot be read is reported and skipped."""
    poses = []
    for f in glob.glob(os.path.join(pose_dir, "*.json")):
        try:
            with open(f, "r") as fp:
                data = json.load(fp)
            stem = os.path.splitext(os.path.basename(f))[0]
            poses.append({"ts": str(data["ts"]) if "ts" in data else stem, "filename_ts": stem,
                          "x": data["x"], "y": data["y"], "z": data["z"],
                          "q": [data["qx"], data["qy"], data["qz"], data["qw"]]})
        except Exception as e:
            print(f"Error loading pose {f}: {e}")
    poses.sort(key=lambda p: p["filename_ts"])
    return poses


def poses_xyzq(poses, indices=None):
    """(S,7) float64 x y z qx qy qz qw of load_poses' dicts (all of them, or those at indices)."""
    if indices is not None:
        poses = [poses[int(i)] for i in indices]
    return np.array([[p["x"], p["y"], p["z"], *p["q"]] for p in poses], dtype=np.float64).reshape(-1, 7)


def plan_slices(poses, segment_len=SEGMENT_LEN, stride=STRIDE, max_pose_gap=MAX_POSE_GAP):
    """Pose index of every slice the reference cuts (:229-245,280).  poses: load_poses' list or an
    array whose first column is x, in file-name order.  current_x runs from x_min + segment_len/2 in
    steps of stride while < x_max; a step takes the pose nearest in x (the first one on a tie) and
    is skipped when that pose is further than max_pose_gap."""
    if len(poses) == 0:
        return []
    if isinstance(poses[0], dict):
        xs = np.array([p["x"] for p in poses], dtype=np.float64)
    else:
        xs = np.asarray(poses, dtype=np.float64).reshape(len(poses), -1)[:, 0]
    x_min, x_max = float(xs.min()), float(xs.max())
    current_x = x_min + segment_len / 2
    chosen = []
    while current_x < x_max:
        gap = np.abs(xs - current_x)
        j = int(np.argmin(gap))
        if not gap[j] > max_pose_gap:
            chosen.append(j)
        current_x += stride
    return chosen


def load_merged_cloud(drive_dir):
    """drive_dir/merged.pcd as io.load_pcd_data gives it (its dtype), at least 2-D, the columns x y z intensity."""
    from .io import load_pcd_data
    return np.atleast_2d(load_pcd_data(os.path.join(drive_dir, "merged.pcd")))[:, :4]


def load_gt_items(json_path):
    """The drive's GT polylines (:99-130): list of {'category', 'points' (n,3) float64, 'attributes'}
    from items[].position or items[].semantic_line.position; items without vertices are dropped."""
    with open(json_path, "r") as f:
        data = json.load(f)
    items = []
    for item in (data.get("items", []) if isinstance(data, dict) else data):
        raw = []
        if item.get("position"):
            raw = item["position"]
        elif item.get("semantic_line") and "position" in item["semantic_line"]:
            raw = item["semantic_line"]["position"]
        pts = [[p["x"], p["y"], p["z"]] for p in raw]
        if pts:
            items.append({"category": item.get("category", "unknown"), "points": np.array(pts, dtype=np.float64),
                          "attributes": item.get("attributes", {})})
    return items


def xyz_dicts(points):
    """(n,3) -> the scene JSON's list of {'x', 'y', 'z'}."""
    return [{"x": float(p[0]), "y": float(p[1]), "z": float(p[2])} for p in points]


def _write_scene_json(json_path, items, ref_ts):
    """write_scene's JSON file (slice_drive writes the .pcd files through pcd.write_pcds)."""
    output = {"timestamp": ref_ts, "items": []}
    for item in items:
        entry = {"category": item["category"], "attributes": item["attributes"], "position": xyz_dicts(item["points"])}
        if "noisy_candidates" in item:
            entry["noisy_candidates"] = [xyz_dicts(c) for c in item["noisy_candidates"]]
        output["items"].append(entry)
    with open(json_path, "w") as f:
        json.dump(output, f, indent=4)


def write_scene(pcd_path, json_path, points, items, ref_ts):
    """The reference's scene files (save_pcd :184-190, save_json :192-209), byte for byte: an ASCII
    PCD of '%.4f %.4f %.4f %d' rows (intensity truncated as int() does) and a JSON of timestamp +
    items[].category / attributes / position, indent 4.  items: dicts with 'category',
    'attributes', 'points' (n,3); an item that carries 'noisy_candidates' (list of (n,3)) gets that
    key too, in the layout augment_train_data.py writes."""
    write_pcd_host(pcd_path, points)
    _write_scene_json(json_path, items, ref_ts)


# ------------------------------------------------------------------ GPU side
def slice_cloud(cloud, poses_xyzq, segment_len=SEGMENT_LEN, radius=RADIUS):
    """Every slice of a drive in two passes over the cloud (:247-261).

    cloud (P,4) float32 xyz + intensity, numpy or CUDA tensor; poses_xyzq (S,7) float64.  Returns
    (points (T,4) float64 CUDA, offsets (S+1,) int64 CUDA, source_index (T,) int64 CUDA): slice s is
    points[offsets[s]:offsets[s+1]] - local xyz and the untouched intensity of the points with
    float32 (x - f32(pose.x))^2 + (y - f32(pose.y))^2 < radius^2 and -segment_len/2 <= local x <=
    segment_len/2, in cloud order; source_index is the cloud row of each.  Bitwise reproducible."""
    dev = G.device("drive")
    cl = G.as_cuda(cloud if torch.is_tensor(cloud) else np.asarray(cloud, dtype=np.float32), dev, "slice_cloud")
    if cl.dtype != torch.float32 or cl.dim() != 2 or cl.shape[1] != 4:
        raise ValueError(f"slice_cloud: cloud must be (P,4) float32, got {tuple(cl.shape)} {cl.dtype}")
    dev = cl.device
    ps = G.poses(poses_xyzq, dev, "slice_cloud")
    npts, n_s = cl.shape[0], ps.shape[0]
    if npts >= 2 ** 31:
        raise ValueError("slice_cloud: at most 2^31 - 1 points per call")
    lib = L.lib()
    nb = lib.prh_drive_slice_workspace_bytes(npts, n_s)
    ws = G.workspace(nb, dev)
    offsets = torch.empty((n_s + 1,), dtype=torch.int64, device=dev)
    L.check(lib.prh_drive_slice_count(G.ptr(cl), npts, G.ptr(ps), n_s, float(segment_len), float(radius), G.ptr(offsets),
                                      G.ptr(ws), nb, dev.index, G.stream(dev)), "prh_drive_slice_count")
    total = int(offsets[-1].item())
    points = torch.empty((total, 4), dtype=torch.float64, device=dev)
    index = torch.empty((total,), dtype=torch.int64, device=dev)
    L.check(lib.prh_drive_slice_write(G.ptr(cl), npts, G.ptr(ps), n_s, float(segment_len), float(radius), G.ptr(offsets),
                                      G.ptr(points), G.ptr(index), total, G.ptr(ws), nb, dev.index, G.stream(dev)),
            "prh_drive_slice_write")
    return points, offsets, index


def clip_lines(lines, poses_xyzq, segment_len=SEGMENT_LEN, return_counts=False):
    """Every polyline of lines (list of (n,3)) in every slice frame, clipped to |x| <= segment_len/2
    with clip_polyline_by_x (:145-182).  Returns, per slice, the list of (line index, (k,3) float64)
    the reference keeps (k > 1, :267-273), in line order.  return_counts=True also returns the
    (S, n_lines) int array of output vertex counts before that rule."""
    ps = G.poses(poses_xyzq, G.device("drive"), "clip_lines")
    return G.clip_two_pass(("prh_drive_clip_workspace_bytes", "prh_drive_clip_count", "prh_drive_clip_write"), lines, ps,
                           segment_len, return_counts)


def _noise(lines, scales, seed, line_ids, draws, dev):
    """(out (K,V,3), draws_u (L,K,4), draws_j (K,V,3)) CUDA float64 and the host CSR offsets."""
    verts, off_t, off = G.lines_csr(lines, dev)
    n_l, n_v = len(lines), int(off[-1])
    k = len(scales) if draws is None else int(draws[0].shape[1])
    if not 1 <= k <= MAX_SCALES:
        raise ValueError(f"drive: 1..{MAX_SCALES} noise scales per call, got {k}")
    vline = torch.from_numpy(np.repeat(np.arange(n_l, dtype=np.int32), np.diff(off))).to(dev)
    ids = None if line_ids is None else torch.from_numpy(np.ascontiguousarray(line_ids, dtype=np.int32)).to(dev)
    if draws is None:
        du = torch.zeros((n_l, k, 4), dtype=torch.float64, device=dev)
        dj = torch.zeros((k, n_v, 3), dtype=torch.float64, device=dev)
    else:
        du, dj = draws
    out = torch.empty((k, n_v, 3), dtype=torch.float64, device=dev)
    sc = (C.c_double * MAX_SCALES)(*([float(s) for s in scales] if draws is None else []))
    lib = L.lib()
    nb = lib.prh_drive_noise_workspace_bytes(n_l)
    ws = G.workspace(nb, dev)
    L.check(lib.prh_drive_noise(G.ptr(verts), G.ptr(off_t), G.ptr(vline), n_v, n_l, G.ptr(ids), sc, k,
                                C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), 1 if draws is None else 0, G.ptr(du),
                                G.ptr(dj), G.ptr(out), G.ptr(ws), nb, dev.index, G.stream(dev)), "prh_drive_noise")
    return out, du, dj, off


def apply_noise(gt, yaw_rad, shift, jitter):
    """The deterministic half of generate_noisy_line (augment_train_data.py:18-54), fp64 on the GPU:
    (gt - centroid) @ R(yaw).T + centroid + shift + jitter with R = [[c,-s,0],[s,c,0],[0,0,1]].
    gt, jitter (n,3); shift (3,).  Returns (n,3) numpy."""
    dev = G.device("drive")
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 3)
    jitter = np.asarray(jitter, dtype=np.float64).reshape(-1, 3)
    if len(jitter) != len(gt):
        raise ValueError("apply_noise: jitter needs one row per vertex")
    du = torch.from_numpy(np.concatenate(([float(yaw_rad)], np.asarray(shift, dtype=np.float64).reshape(3)))
                          .reshape(1, 1, 4)).to(dev)
    dj = torch.from_numpy(np.ascontiguousarray(jitter).reshape(1, -1, 3)).to(dev)
    out, _, _, _ = _noise([gt], (), 0, None, (du, dj), dev)
    return out[0].cpu().numpy()


def noisy_candidates(gt_lines, noise_scales=NOISE_SCALES, seed=0, return_draws=False):
    """len(noise_scales) noisy candidates of every GT line (generate_noisy_line, augment :18-54):
    per (line, scale s) yaw ~ U(+-5 deg * s), dx, dy ~ U(+-s), dz ~ U(+-0.1), per-vertex jitter
    N(0, 0.05) in x, y and N(0, 0.025) in z, drawn on the device from a counter hash of (seed, line,
    candidate, vertex, component), then apply_noise.  Returns a list (per line) of lists (per scale)
    of (n,3) numpy arrays; the same seed gives the same bits.  return_draws=True also returns
    {'yaw' (L,K) rad, 'shift' (L,K,3), 'jitter' [per line (K,n,3)]}.  Same distribution as the
    reference's numpy draws, not the same numbers."""
    dev = G.device("drive")
    out, du, dj, off = _noise(gt_lines, tuple(noise_scales), seed, None, None, dev)
    out, du, dj = out.cpu().numpy(), du.cpu().numpy(), dj.cpu().numpy()
    k = len(noise_scales)
    cands = [[out[c, off[l]:off[l + 1]].copy() for c in range(k)] for l in range(len(gt_lines))]
    if not return_draws:
        return cands
    draws = {"yaw": du[:, :, 0].copy(), "shift": du[:, :, 1:].copy(),
             "jitter": [dj[:, off[l]:off[l + 1]].copy() for l in range(len(gt_lines))]}
    return cands, draws


def stream_candidates(gt_lines, item_ids, noise_scales, seed, device):
    """SceneSampleStream's per-epoch draw: candidates of gt_lines hashed under their item numbers.
    Returns out[k][l] as a list (per scale) of lists (per line) of (n,3) numpy arrays."""
    dev = G.device("drive", device)
    out, _, _, off = _noise(gt_lines, tuple(noise_scales), seed, item_ids, None, dev)
    out = out.cpu().numpy()
    return [[out[c, off[l]:off[l + 1]] for l in range(len(gt_lines))] for c in range(len(noise_scales))]


def slice_drive(drive_dir, gt_json, out_dir=None, candidates=False, noise_scales=NOISE_SCALES, seed=0,
                segment_len=SEGMENT_LEN, stride=STRIDE, radius=RADIUS, max_pose_gap=MAX_POSE_GAP, verbose=True):
    """process_dataset (:211-282) for one drive: drive_dir holds pose/*.json and merged.pcd, gt_json
    the GT polylines.  One slice_cloud and one clip_lines call serve every slice.  With out_dir the
    scene files NAME.pcd / NAME.json (NAME = the pose's file name) are written; candidates=True adds
    noisy_candidates drawn on the device (seeded per slice) the way augment_train_data.py stores
    them.  A slice that keeps no point is not written (the reference skips a slice whose 60 m disc
    is empty and writes an empty file when only the crop is).  Returns {'pose_index', 'names',
    'points' (T,4) CUDA, 'offsets', 'source_index', 'items' [per slice list of item dicts],
    'written' [names]}."""
    poses = load_poses(os.path.join(drive_dir, "pose"))
    res = {"pose_index": [], "names": [], "points": None, "offsets": None, "source_index": None, "items": [],
           "written": []}
    if not poses:
        if verbose:
            print("  No poses found. Skipping.")
        return res
    cloud = load_merged_cloud(drive_dir)
    if len(cloud) == 0:
        if verbose:
            print("  No points found. Skipping.")
        return res
    gt_items = load_gt_items(gt_json) if os.path.exists(gt_json) else []
    xs = [p["x"] for p in poses]
    if verbose:
        print(f"  Path X range: {min(xs):.1f} to {max(xs):.1f} ({max(xs) - min(xs):.1f}m)")
    chosen = plan_slices(poses, segment_len, stride, max_pose_gap)
    pq = poses_xyzq(poses, chosen)
    points, offsets, index = slice_cloud(cloud.astype(np.float32, copy=False), pq, segment_len, radius)
    clipped = clip_lines([it["points"] for it in gt_items], pq, segment_len)
    off = offsets.cpu().numpy()
    res.update(pose_index=chosen, names=[poses[j]["filename_ts"] for j in chosen], points=points, offsets=offsets,
               source_index=index)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    pcd_paths = [None] * len(res["names"])
    for s, name in enumerate(res["names"]):
        items = [{"category": gt_items[l]["category"], "points": v, "attributes": gt_items[l]["attributes"]}
                 for l, v in clipped[s]]
        if candidates and items:
            cands = noisy_candidates([it["points"] for it in items], noise_scales, seed=int(seed) * 1000003 + s)
            for it, c in zip(items, cands):
                it["noisy_candidates"] = c
        res["items"].append(items)
        if out_dir is not None and off[s + 1] > off[s]:
            pcd_paths[s] = os.path.join(out_dir, f"{name}.pcd")
            _write_scene_json(os.path.join(out_dir, f"{name}.json"), items, name)
            res["written"].append(name)
    if out_dir is not None:
        write_pcds(pcd_paths, points, off)              # the text of every slice from one device pass
    if verbose:
        print(f"  Generated {len(res['written']) if out_dir is not None else int((np.diff(off) > 0).sum())} samples.")
    return res
