"""Plain numpy restatement of the context builder's crop, order and draw (csrc/prh_context.hpp),
and the generators of the inputs that test_context_exact_cpu.py (conditions on the inputs) and
test_context_exact_gpu.py (the kernels) share.

The draw is a function of (seed, line index within the call, cloud index) through a splitmix64
hash that np.uint64 reproduces bit for bit, so which points a call returns can be restated and
compared by index instead of in distribution:
  K <= N : row i is candidate  hash(seed, line, 0x40000000 + i) % K           - exact integers
  K >  N : the N largest keys  log w + G,  G = -log(-log u),  u = u01(hash(seed, line, index)),
           returned in cloud order.  The kernel's keys are fp32, these are fp64: selection_bounds
           gives the set every correct kernel must return and the set it may return, which differ
           only by keys within 2 eps of the N-th / (N+1)-th largest.
Point identity: the generators give point i the intensity float(perm[i]) (a permutation of 0..P-1,
P < 2^24), so column 3 of an output row names the cloud index; flat-intensity inputs carry a
unique x instead."""
import functools

import numpy as np

from oracle import context_oracle as O

U64 = np.uint64
_MASK = (1 << 64) - 1
EPS_KEY = 1e-4            # fp32 key against fp64 key: 3e-5 (the weight tolerance, as a shift of log w)
                          # + < 2e-5 (logf rounding at |key| <= 40 and the rounded sum), rest margin
ZERO_CLASS = 2.0 ** -150  # below half the smallest fp32 subnormal: expf gives 0, the key is -3e38
WITH_REPLACEMENT_BASE = 0x40000000


# ------------------------------------------------------------------ the hash and the uniform
def mix64(x):
    """splitmix64 finaliser on np.uint64 (wrap-around arithmetic)."""
    x = np.asarray(x, dtype=U64)
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def ctx_hash(seed, line, idx):
    """hash of (seed, line, idx): seed any Python int (taken mod 2^64), line and idx < 2^32."""
    v = (U64(int(line)) << U64(32)) | np.asarray(idx, dtype=np.int64).astype(U64)
    return mix64(mix64(U64(int(seed) & _MASK) ^ v))


def u01(h):
    """The kernel's uniform: ((float)(h >> 41) + 0.5f) * 2^-23 - every step exact in float32."""
    k = (np.asarray(h, dtype=U64) >> U64(41)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(1.0 / 8388608.0)


def u01_24bit(h):
    """The formula the kernel used before: 24 bits do not fit float32 once 0.5 is added."""
    k = (np.asarray(h, dtype=U64) >> U64(40)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


# ------------------------------------------------------------------ crop, weights, keys
def f32(x):
    """The value a float32 kernel argument has, as a Python float."""
    return float(np.float32(x))


def crop_indices(cloud, dense, radius):
    """Cloud indices inside the tube, in cloud order: fp64 distance to the nearest polyline sample,
    strict < (oracle.context_oracle.crop_mask)."""
    if len(cloud) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.nonzero(O.crop_mask(np.asarray(cloud), np.asarray(dense, dtype=np.float64), radius))[0]


def weights64(cands, line, decay):
    return O.sampling_weights(np.asarray(cands, dtype=np.float64), np.asarray(line, dtype=np.float64), decay)


def keys64(w, seed, line_index, cloud_idx):
    """Gumbel-top-k keys in fp64: log w + g, g alone when the weights sum to < 1e-6, -inf for a
    weight of the zero class."""
    w = np.asarray(w, dtype=np.float64)
    u = u01(ctx_hash(seed, line_index, cloud_idx)).astype(np.float64)
    g = -np.log(-np.log(u))
    if w.sum() < 1e-6:
        return g
    with np.errstate(divide="ignore"):
        return np.where(w < ZERO_CLASS, -np.inf, np.log(np.maximum(w, 1e-320)) + g)


def expected_with_replacement(seed, line_index, K, N):
    """Candidate positions (into the crop list) of the N rows of a K <= N draw."""
    h = ctx_hash(seed, line_index, WITH_REPLACEMENT_BASE + np.arange(N, dtype=np.int64))
    return (h % U64(K)).astype(np.int64)


def selection_bounds(keys, N, eps=EPS_KEY):
    """(must, may): positions a correct top-N selection of len(keys) > N keys has to contain / may
    contain when each key is known to within eps.  -inf keys tie; the first in cloud order win."""
    keys = np.asarray(keys, dtype=np.float64)
    assert len(keys) > N >= 1
    finite = np.isfinite(keys)
    n_fin = int(finite.sum())
    if n_fin < N:
        must = finite.copy()
        must[np.nonzero(~finite)[0][:N - n_fin]] = True
        return np.nonzero(must)[0], np.nonzero(must)[0]
    desc = np.sort(keys)[::-1]
    k_n, k_n1 = desc[N - 1], desc[N]
    must = keys > k_n1 + 2 * eps            # k_n1 = -inf when exactly N keys are finite: all of them
    may = finite & (keys >= k_n - 2 * eps)
    return np.nonzero(must)[0], np.nonzero(may)[0]


def boundary_band(cloud, dense_lines, radius):
    """Indices of points whose fp64 distance to any of the lines is within 1e-5 max(1, r) of r:
    three orders above the fp32 fma rounding of d^2, so the crop set is the same in both precisions."""
    bad = np.zeros(len(cloud), dtype=bool)
    for d in dense_lines:
        if len(cloud):
            dist = O.nearest_distance(np.asarray(cloud)[:, :3], np.asarray(d, dtype=np.float64))
            bad |= np.abs(dist - radius) < 1e-5 * max(1.0, radius)
    return np.nonzero(bad)[0]


def mean_tolerance(m, *coords):
    """Sequential fp32 mean over m points + one subtraction: (m + 2) 2^-24 max|coordinate|."""
    return (m + 2) * 2.0 ** -24 * max(float(np.abs(c).max()) if np.size(c) else 0.0 for c in coords)


# ------------------------------------------------------------------ inputs
class Case:
    """One call: float32 arrays cloud (P,4), dense (L,D,3), line (L,M,3), the float32 values of
    radius and decay, and whatever the generator promises about it (k = points per tube, ...)."""

    def __init__(self, name, cloud, dense, line, radius, decay, **promise):
        self.name = name
        self.cloud = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4)
        self.dense = np.ascontiguousarray(dense, dtype=np.float32)
        self.line = np.ascontiguousarray(line, dtype=np.float32)
        self.radius, self.decay = f32(radius), f32(decay)
        self.promise = promise
        self._dist, self._w = {}, {}

    @property
    def n_lines(self):
        return self.dense.shape[0]

    def dist(self, l):
        """fp64 distance of every cloud point to line l's dense samples, computed once; inf for the
        points outside the samples' bounding box grown by 1.001 r + 1e-3 (farther than r and than
        the boundary band from every sample, so crop and band do not depend on the shortcut)."""
        if l not in self._dist:
            d = np.full(len(self.cloud), np.inf)
            dense = self.dense[l].astype(np.float64)
            grow = 1.001 * self.radius + 1e-3
            xyz = self.cloud[:, :3]
            box = np.all((xyz >= dense.min(0) - grow) & (xyz <= dense.max(0) + grow), axis=1)
            if box.any():
                d[box] = O.nearest_distance(xyz[box], dense)
            self._dist[l] = d
        return self._dist[l]

    def move(self, idx, xyz):
        """Replace the coordinates of the points idx (generators: re-drawing the boundary band)."""
        self.cloud[idx, :3] = np.asarray(xyz, dtype=np.float32)
        self._dist, self._w = {}, {}

    def crop(self, l):
        return np.nonzero(self.dist(l) < self.radius)[0]          # = crop_indices(cloud, dense[l], radius)

    def weights(self, l):
        if l not in self._w:
            self._w[l] = weights64(self.cloud[self.crop(l)], self.line[l], self.decay)
        return self._w[l]

    def keys(self, l, seed):
        return keys64(self.weights(l), seed, l, self.crop(l))

    def band(self):
        """= boundary_band(cloud, dense, radius), from the cached distances."""
        bad = np.zeros(len(self.cloud), dtype=bool)
        for l in range(self.n_lines):
            bad |= np.abs(self.dist(l) - self.radius) < 1e-5 * max(1.0, self.radius)
        return np.nonzero(bad)[0]

    def centre(self, l):
        return self.line[l].astype(np.float64).mean(0)


def _identity(rng, xyz):
    """(P,4) cloud whose intensity column is a fixed permutation of 0..P-1."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    return np.column_stack([xyz, rng.permutation(len(xyz)).astype(np.float64)])


def _settle(case, redraw):
    """Empty the boundary band: the few points that fall into it are drawn again in place
    (redraw(indices) -> new xyz), which keeps the cloud's size and every other point's index."""
    for _ in range(20):
        bad = case.band()
        if len(bad) == 0:
            return case
        case.move(bad, redraw(bad))
    raise AssertionError(f"{case.name}: boundary band not empty")


def _poly(raw, n):
    raw = np.asarray(raw, dtype=np.float64)
    return raw[:1].copy() if n == 1 else O.arc_resample(raw, n)


def _lines(raws, nd=200, m=32):
    dense = np.stack([_poly(r, nd) for r in raws]).astype(np.float32)
    line = np.stack([_poly(r, m) for r in raws]).astype(np.float32)
    return dense, line


BENT = [[-10.0, -4.0, 0.0], [0.0, 4.0, 0.0], [10.0, -4.0, 0.0]]     # its box is mostly decoys
SLANT = [[-10.0, 1.0, 0.0], [10.0, -1.0, 0.0]]
SWEEP_NPTS = (1, 255, 256, 257, 65536, 65537)


@functools.lru_cache(maxsize=None)
def sweep_case(npts, nd=200, m=32):
    """A wide sheet of points under a bent and a slanted line (they cross: overlapping tubes).  The
    bent line's bounding box spans the sheet while its tube covers ~ 1/8 of it."""
    rng = np.random.default_rng(1000 + npts + 7 * nd + 13 * m)
    radius = 0.7
    dense, line = _lines([BENT, SLANT], nd, m)
    sheet = lambda n: np.column_stack([rng.uniform(-12, 12, n), rng.uniform(-6, 6, n), rng.normal(0, 0.05, n)])
    xyz = sheet(npts)
    if npts == 1:
        xyz[:, :2] = [0.1, 3.8]                                  # under the apex of the bent line only
    case = Case(f"sweep{npts}_d{nd}_m{m}", _identity(rng, xyz), dense, line, radius, 2.0)
    return _settle(case, lambda idx: sheet(len(idx)))


LIMIT_SHAPES = ((1, 1), (200, 32), (256, 64), (1, 64), (256, 1))
LIMIT_NPTS = 3000                   # enough for a dozen points in the ball that n_dense = 1 leaves of a tube


STRUCT_NPTS = 66000                 # 258 blocks, the last one partial (208 points); scan: 2 blocks per thread
STRUCT_ROLES = ("last_block_only", "first_and_last_block", "empty", "everything", "bent", "crossing")


@functools.lru_cache(maxsize=None)
def structured_case():
    """Six lines over one strip of points (|y| < 0.9 around the x axis, radius 1):
      0  a short line at x ~ 51: only points of the last, partial block lie near it
      1  a short line at x ~ 41: only points of the first and of the last block lie near it, every
         block between leaves at the bounding-box test
      2  a line 500 m away: no point
      3  the axis of the strip: every point
      4, 5  a bent and a straight line through the bulk, overlapping each other (and 3)."""
    rng = np.random.default_rng(77)
    radius = 1.0
    raws = [[[50.0, 0.0, 0.0], [52.0, 0.0, 0.0]],
            [[40.0, 0.0, 0.0], [42.0, 0.0, 0.0]],
            [[0.0, 500.0, 0.0], [30.0, 500.0, 0.0]],
            [[-10.0, 0.0, 0.0], [60.0, 0.0, 0.0]],
            [[0.0, -0.8, 0.0], [15.0, 0.8, 0.0], [30.0, -0.8, 0.0]],
            [[10.0, 0.3, 0.0], [20.0, 0.3, 0.0]]]
    dense, line = _lines(raws)
    P = STRUCT_NPTS
    last0 = (P // 256) * 256

    def zone(n, x0, x1):
        return np.column_stack([rng.uniform(x0, x1, n), rng.uniform(-0.9, 0.9, n), rng.normal(0, 0.02, n)])

    xyz = zone(P, -9.0, 37.0)                                    # bulk: clear of lines 0 and 1
    first = rng.choice(256, 90, replace=False)
    xyz[first] = zone(90, 40.3, 41.7)                            # block 0 -> line 1
    tail = last0 + rng.permutation(P - last0)
    xyz[tail[:70]] = zone(70, 40.3, 41.7)                        # last block -> line 1
    xyz[tail[70:150]] = zone(80, 50.3, 51.7)                     # last block -> line 0
    case = Case("structured", _identity(rng, xyz), dense, line, radius, 2.0, last_block_start=last0)

    def redraw(idx):                                             # same x (same zone), new y and z
        new = case.cloud[idx, :3].astype(np.float64)
        new[:, 1:] = zone(len(idx), 0, 1)[:, 1:]
        return new
    return _settle(case, redraw)


# four parallel lanes 10 m apart; lane l's tube gets exactly k[l] points, everything else is >= 2 m away
_LANE_Y = (0.0, 10.0, 20.0, 30.0)


def _lane_raw(y):
    return [[-5.0, y, 0.0], [5.0, y, 0.0]]


def _lane_cloud(rng, ks, radius, ylo, yhi, lanes, spare_outside, flat=False, near_frac=0.0):
    """ks[l] points at lateral offset ylo..yhi (either side) of lane l, `spare_outside` points between
    the lanes; shuffled, so that the candidates of every lane are spread over the whole cloud."""
    parts = []
    for k, y in zip(ks, lanes):
        off = rng.uniform(ylo, yhi, k) * rng.choice([-1.0, 1.0], k)
        parts.append(np.column_stack([rng.uniform(-4.5, 4.5, k), y + off, rng.normal(0, 0.01, k)]))
    out = np.column_stack([rng.uniform(-6, 6, spare_outside), rng.choice(lanes, spare_outside) + 5.0
                           + rng.uniform(-2.5, 2.5, spare_outside), rng.normal(0, 0.01, spare_outside)])
    xyz = np.concatenate(parts + [out])
    if flat:                                                     # unique x names the point
        xyz[:, 0] = -4.5 + 9.0 * (rng.permutation(len(xyz)) + rng.uniform(0.2, 0.8, len(xyz))) / len(xyz)
    return xyz[rng.permutation(len(xyz))]


DRAW_SHAPES = ((2, 1), (256, 255), (257, 256), (258, 257), (257, 6), (511, 256), (513, 64), (1000, 999),
               (5000, 1024))
DRAW_SEEDS = (0, 1, 2 ** 40 + 3, 2 ** 64 - 1)
# generator seeds: the first of 0, 1, 2, ... at which the 1 % ambiguity cap holds for all DRAW_SEEDS
# (test_context_exact_cpu.py checks the cap; it is a condition on the inputs)
DRAW_GEN_SEED = {}


@functools.lru_cache(maxsize=None)
def draw_case(K, N, same_line=False):
    """Exactly K points in each of four tubes (same_line: one tube, the same line four times)."""
    rng = np.random.default_rng(5000 + 31 * K + N + DRAW_GEN_SEED.get((K, N, same_line), 0))
    lanes = (_LANE_Y[0],) if same_line else _LANE_Y
    xyz = _lane_cloud(rng, [K] * len(lanes), 0.5, 0.0, 0.4, lanes, K // 2 + 37)
    dense, line = _lines([_lane_raw(y) for y in (lanes * 4)[:4]])
    return Case(f"draw_K{K}_N{N}" + ("_same" if same_line else ""), _identity(rng, xyz), dense, line, 0.5, 0.25,
                k=[K] * 4, n=N)


@functools.lru_cache(maxsize=None)
def flat_case():
    """Flat intensity (7.0 everywhere): the weight is exp(-d/decay); unique x per point."""
    rng = np.random.default_rng(61)
    K, N = 1000, 300
    xyz = _lane_cloud(rng, [K] * 4, 0.5, 0.0, 0.4, _LANE_Y, 537, flat=True)
    dense, line = _lines([_lane_raw(y) for y in _LANE_Y])
    cloud = np.column_stack([xyz, np.full(len(xyz), 7.0)])
    return Case("flat", cloud, dense, line, 0.5, 0.25, k=[K] * 4, n=N)


@functools.lru_cache(maxsize=None)
def uniform_case():
    """decay 0.02 and every candidate >= 0.5 m from the line points: the weights sum to < 1e-6."""
    rng = np.random.default_rng(62)
    K, N = 1000, 256
    xyz = _lane_cloud(rng, [K] * 4, 1.0, 0.55, 0.9, _LANE_Y, 537)
    dense, line = _lines([_lane_raw(y) for y in _LANE_Y])
    return Case("uniform", _identity(rng, xyz), dense, line, 1.0, 0.02, k=[K] * 4, n=N)


@functools.lru_cache(maxsize=None)
def zero_case(n_pos, n_zero, N=256):
    """decay 0.005, radius 1: n_pos candidates within 0.3 m of the axis (d/decay <= 80, a tenth of
    them within 1 cm of a line point so that the sum stays >= 1e-6) and n_zero at 0.65..0.9 m
    (d/decay >= 120: expf gives 0)."""
    rng = np.random.default_rng(63 + n_pos)
    lanes = _LANE_Y
    dense, line = _lines([_lane_raw(y) for y in lanes])
    parts = []
    for l, y in enumerate(lanes):
        pos = np.column_stack([rng.uniform(-4.5, 4.5, n_pos), y + rng.uniform(-0.3, 0.3, n_pos), np.zeros(n_pos)])
        near = max(3, n_pos // 10)
        pos[:near] = line[l][rng.integers(0, 32, near)].astype(np.float64) + rng.uniform(-0.005, 0.005, (near, 3))
        zer = np.column_stack([rng.uniform(-4.5, 4.5, n_zero),
                               y + rng.uniform(0.65, 0.9, n_zero) * rng.choice([-1.0, 1.0], n_zero), np.zeros(n_zero)])
        parts += [pos, zer]
    out = np.column_stack([rng.uniform(-6, 6, 300), rng.choice(lanes, 300) + 5.0 + rng.uniform(-2.5, 2.5, 300),
                           np.zeros(300)])
    xyz = np.concatenate(parts + [out])
    xyz = xyz[rng.permutation(len(xyz))]
    return Case(f"zero_{n_pos}_{n_zero}", _identity(rng, xyz), dense, line, 1.0, 0.005,
                k=[n_pos + n_zero] * 4, n=N, n_pos=n_pos)


REPLACE_N = (1, 40, 257, 1024)


@functools.lru_cache(maxsize=None)
def replace_case(N):
    """K <= N: lanes with K = N, N - 1, 1 and 0 points."""
    rng = np.random.default_rng(7000 + N)
    ks = [N, N - 1, 1, 0]
    xyz = _lane_cloud(rng, ks, 0.5, 0.0, 0.4, _LANE_Y, N // 2 + 37)
    dense, line = _lines([_lane_raw(y) for y in _LANE_Y])
    return Case(f"replace_N{N}", _identity(rng, xyz), dense, line, 0.5, 0.25, k=ks, n=N)


BRANCH_N = (40, 257)


@functools.lru_cache(maxsize=None)
def branch_pair(N):
    """Two clouds that differ in one point: K = N + 1 (weighted, without replacement) and, with
    that point moved out of the tube, K = N (uniform, with replacement)."""
    rng = np.random.default_rng(8000 + N)
    xyz = _lane_cloud(rng, [N + 1] * 4, 0.5, 0.0, 0.4, _LANE_Y, N // 2 + 37)
    dense, line = _lines([_lane_raw(y) for y in _LANE_Y])
    cloud = _identity(rng, xyz)
    more = Case(f"branch_N{N}_more", cloud, dense, line, 0.5, 0.25, k=[N + 1] * 4, n=N)
    fewer_cloud = cloud.copy()
    for l in range(4):                                   # the middle candidate of every lane leaves
        fewer_cloud[more.crop(l)[N // 2], 1] += 5.0
    fewer = Case(f"branch_N{N}_fewer", fewer_cloud, dense, line, 0.5, 0.25, k=[N] * 4, n=N)
    return more, fewer


@functools.lru_cache(maxsize=None)
def retry_case():
    """One tube of 9000 points: more than the default candidate buffer (8192 slots) holds."""
    rng = np.random.default_rng(91)
    xyz = _lane_cloud(rng, [9000], 0.5, 0.0, 0.4, (0.0,), 1200)
    dense, line = _lines([_lane_raw(0.0)])
    return Case("retry", _identity(rng, xyz), dense, line, 0.5, 0.25, k=[9000], n=1024)


def ambiguity(case, seed, N, lines=None):
    """sum over the lines with K > N of |may \\ must|."""
    tot = 0
    for l in (range(case.n_lines) if lines is None else lines):
        if len(case.crop(l)) > N:
            must, may = selection_bounds(case.keys(l, seed), N)
            tot += len(may) - len(must)
    return tot
