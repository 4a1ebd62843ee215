"""Edge tables and plain references of the 64-lane primitives probed by pdmp_debug_wave_eval (include/pdmp_debug.h: PDMP_WAVE_*).

A table is [nrows x 64] u64 words (bit images of doubles, or u32 in the low half); one wavefront evaluates a row.  reference(name, in0, in1)
restates the operation in numpy -- what a lane must hold afterwards, from the function's comment, never from its code -- and returns
(words, mask): mask marks the lanes the comment promises something about AND whose value the contract fixes (a minimum over NaN lanes only is
left out).  same(name, dev, ref) is the comparison the GPU tests use: bit for bit, except that a zero minimum may carry either sign.
tests/test_wave_queue_tables_ref.py checks the references against their invariants on every row, so the tables are known good before a device
sees them.
"""
import numpy as np

IDS = {"PDMP_WAVE_MIN_F64": 0, "PDMP_WAVE_GRP8_MIN_F64": 1, "PDMP_WAVE_ROW_MIN_F64": 2, "PDMP_WAVE_MIN_U32": 3, "PDMP_WAVE_MIN_U32_DPP": 4,
       "PDMP_WAVE_SCAN_ADD_U32": 5, "PDMP_WAVE_SCAN_MIN_F64": 6, "PDMP_WAVE_BPERM_F64": 7, "PDMP_WAVE_SUM_F64": 8, "PDMP_WAVE_GRP8_MIN_U32": 9}
MIN_F64 = {"PDMP_WAVE_MIN_F64": 64, "PDMP_WAVE_GRP8_MIN_F64": 8, "PDMP_WAVE_ROW_MIN_F64": 16}  # name -> lanes of a group
MIN_U32 = {"PDMP_WAVE_MIN_U32": 64, "PDMP_WAVE_MIN_U32_DPP": 64, "PDMP_WAVE_GRP8_MIN_U32": 8}

QNAN = np.uint64(0x7FF8000000000000)  # quiet NaN only: in IEEE mode a signalling NaN is answered with a NaN
INF = np.inf
DENORM_MIN = 5e-324
LANES = np.arange(64)
PREFIXES = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63)  # leading lanes that hold the identity: every DPP step's boundary


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _f64(w):
    return np.ascontiguousarray(w, dtype=np.uint64).view(np.float64)


# ------------------------------------------------------------------------------------------------ tables

def f64_min_rows():
    """rows for the f64 minima and the prefix minimum"""
    rng = np.random.default_rng(0x5EED)
    rows = []
    for L in range(64):  # one-hot: the minimum in lane L, for every L -- any wrong control code, row mask or bank mask skips some lane
        r = np.full(64, 5.0)
        r[L] = -3.0
        rows.append(r)
    for L in range(64):  # ... and every lane different, the minimum in lane L (a wrong source lane shows even where it is not the minimum's)
        r = 100.0 + ((LANES * 37 + 11) % 64).astype(np.float64)
        r[L] = 1.5
        rows.append(r)
    for v in (1.5, -2.0, 0.0, -0.0, 1e300, -1e300, DENORM_MIN, INF, -INF):  # constant rows (+Inf everywhere among them)
        rows.append(np.full(64, v))
    for lanes in ((3, 17, 40), (0, 63), (7, 8), (15, 16, 31, 32, 47, 48), (0, 1, 2, 3), tuple(range(0, 64, 8)), tuple(range(7, 64, 8))):  # ties
        r = 10.0 + LANES
        r[list(lanes)] = -7.25
        rows.append(r)
    rows.append(64.0 - LANES)  # strictly decreasing
    rows.append(LANES - 31.5)  # strictly increasing
    rows.append(-(1.0 + LANES * 2.0**-52))  # ... one ulp apart
    rows.append(1.0 + LANES * 2.0**-52)
    for k in PREFIXES:  # the first k lanes hold the identity
        r = rng.standard_normal(64)
        r[:k] = INF
        rows.append(r)
    for _ in range(32):
        rows.append(rng.standard_normal(64))
    for _ in range(8):  # all magnitudes and signs
        rows.append(rng.standard_normal(64) * 2.0 ** rng.integers(-1000, 1000, 64))
    for L in range(64):  # +Inf with one finite lane
        r = np.full(64, INF)
        r[L] = 1e300 if L % 2 else -4.0
        rows.append(r)
    for _ in range(4):  # denormals of both signs, denorm_min among them
        r = _f64(rng.integers(1, 1 << 52, 64).astype(np.uint64)) * rng.choice([-1.0, 1.0], 64)
        r[rng.integers(0, 64)] = DENORM_MIN
        rows.append(r)
    rows.append(np.where(LANES % 3 == 0, DENORM_MIN, 2 * DENORM_MIN))
    rows.append(np.where(LANES % 2 == 0, 0.0, -0.0))  # mixed zeros: the sign of a zero minimum is not promised
    rows.append(np.where(LANES % 5 == 0, -0.0, 0.0))
    rows.append(np.where(LANES % 7 == 3, -0.0, np.where(LANES % 2 == 0, 0.0, 3.0)))
    rows.append(np.where(LANES == 40, -0.0, 1.0 + LANES))
    out = _bits(np.array(rows)).copy()
    nan_rows = []  # quiet NaN in some lanes beside finite ones: NaN loses
    for _ in range(8):
        w = _bits(rng.standard_normal(64)).copy()
        w[rng.random(64) < 0.5] = QNAN
        w[::8][_f64(w[::8]) != _f64(w[::8])] = _bits([2.5])[0]  # (a finite lane in every group of 8)
        nan_rows.append(w)
    for L in (0, 1, 15, 16, 31, 32, 62, 63):  # NaN in every lane but one
        w = np.full(64, QNAN)
        w[L] = _bits([-1.25])[0]
        nan_rows.append(w)
    for L in (0, 5, 63):  # one NaN lane: in the lane of the would-be minimum's neighbour
        w = _bits(10.0 + LANES).copy()
        w[L] = QNAN
        nan_rows.append(w)
    out = np.vstack([out, np.array(nan_rows)])
    return np.ascontiguousarray(out)


def u32_rows():
    rng = np.random.default_rng(0xC0FFEE)
    M = 0xFFFFFFFF
    rows = []
    for L in range(64):  # one-hot against 0xffffffff
        r = np.full(64, M, dtype=np.uint64)
        r[L] = 12345 + L
        rows.append(r)
    for L in range(64):  # every lane different, the minimum in lane L
        r = (1000 + (LANES * 37 + 11) % 64).astype(np.uint64)
        r[L] = 3
        rows.append(r)
    for v in (0, 1, 7, 0x7FFFFFFF, 0x80000000, M):  # constant rows (all 0xffffffff among them)
        rows.append(np.full(64, v, dtype=np.uint64))
    for L in range(0, 64, 3):  # both sides of 2^31: a signed compare takes 0x80000000 for the smallest
        r = np.where(LANES % 2 == 0, 0x80000000, 0x80000001).astype(np.uint64)
        r[L] = 0x7FFFFFFF
        rows.append(r)
    rows.append(np.where(LANES % 2 == 0, 0x7FFFFFFE, 0x80000000).astype(np.uint64))
    rows.append((0x7FFFFFE0 + LANES).astype(np.uint64))  # increasing across 2^31
    rows.append((0x8000001F - LANES).astype(np.uint64))  # decreasing across 2^31
    for lanes in ((3, 17, 40), (0, 63), (7, 8), (15, 16, 31, 32, 47, 48), tuple(range(7, 64, 8))):  # ties
        r = (100 + LANES).astype(np.uint64)
        r[list(lanes)] = 9
        rows.append(r)
    rows.append((64 - LANES).astype(np.uint64))
    rows.append((1 + LANES).astype(np.uint64))
    for k in PREFIXES:  # the first k lanes hold the scan's identity
        r = rng.integers(1, 1000, 64).astype(np.uint64)
        r[:k] = 0
        rows.append(r)
    for _ in range(32):
        rows.append(rng.integers(0, 1 << 32, 64).astype(np.uint64))  # (sums of these wrap past 2^32 many times)
    for _ in range(8):
        rows.append(rng.integers(0, 64, 64).astype(np.uint64))  # small counts, as the kernels scan them
    rows.append(np.full(64, 0x04000000, dtype=np.uint64))  # the sum reaches 2^32 exactly in lane 63
    rows.append(np.where(LANES == 0, M, 1).astype(np.uint64))  # wraps at lane 1
    rows.append(np.where(LANES == 31, M, np.where(LANES == 32, 1, 0)).astype(np.uint64))  # wraps across the row_bcast:31 step
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64))


def bperm_rows():
    """(values, source lanes): arbitrary bit patterns (both halves must travel), sources 0..63 only"""
    rng = np.random.default_rng(0xB9E7)
    srcs = [LANES, 63 - LANES, LANES ^ 1, LANES ^ 32, (LANES + 1) % 64, (LANES + 17) % 64, (LANES * 5) % 64, LANES // 2, np.zeros(64), np.full(64, 63)]
    srcs += [np.full(64, L) for L in (1, 15, 16, 31, 32, 47, 48)]
    srcs += [rng.permutation(64) for _ in range(8)] + [rng.integers(0, 64, 64) for _ in range(8)]
    src = np.array(srcs, dtype=np.uint64)
    val = rng.integers(0, 1 << 64, src.shape, dtype=np.uint64)
    val[0] = _bits(LANES + 0.5)
    val[1] = (LANES.astype(np.uint64) << np.uint64(32)) | (63 - LANES).astype(np.uint64)  # high and low halves tell the lane apart
    return np.ascontiguousarray(val), np.ascontiguousarray(src)


def sum_rows():
    """finite rows for wave_sum_f64; the heavy-cancellation rows make the order of the additions show in the bits"""
    rng = np.random.default_rng(0x50AF)
    rows = []
    for L in range(64):  # one-hot
        r = np.zeros(64)
        r[L] = 1.0 + L
        rows.append(r)
    for v in (0.0, -0.0, 1.0, 0.1, -2.5, 1e300 / 64):
        rows.append(np.full(64, v))
    rows.append(LANES + 1.0)
    rows.append((-1.0) ** LANES)
    for _ in range(32):
        rows.append(rng.standard_normal(64))
    big = np.array([1e16, 1.0, -1e16, 1.0])
    for shift in range(4):  # heavy cancellation: what is left depends on which partial sums meet first
        rows.append(np.roll(np.tile(big, 16), shift))
    for _ in range(24):
        r = rng.standard_normal(64) * 2.0 ** rng.integers(-40, 60, 64)
        p = rng.permutation(64)
        r[p[:24]] = -r[p[24:48]]  # pairs that cancel exactly -- in some orders only
        rows.append(r)
    for stride in (1, 2, 4, 8, 16, 32):  # 2^53 against ones placed a butterfly stride apart
        r = np.ones(64)
        r[::2 * stride] = 2.0**53
        r[stride::2 * stride] = -(2.0**53)
        rows.append(r)
    return _bits(np.array(rows)).copy()


def tables(name):
    """(in0, in1) of probe `name`"""
    if name in MIN_F64 or name == "PDMP_WAVE_SCAN_MIN_F64":
        t = f64_min_rows()
    elif name in MIN_U32 or name == "PDMP_WAVE_SCAN_ADD_U32":
        t = u32_rows()
    elif name == "PDMP_WAVE_BPERM_F64":
        return bperm_rows()
    else:
        assert name == "PDMP_WAVE_SUM_F64", name
        t = sum_rows()
    return t, np.zeros_like(t)


# ------------------------------------------------------------------------------------------------ references

def _grouped_min_f64(v, g):
    """(minimum of the non-NaN lanes of each group of g lanes, in every lane of the group; has the group such a lane)"""
    x = v.reshape(len(v), 64 // g, g)
    ok = ~np.isnan(x)
    m = np.where(ok, x, INF).min(axis=2, keepdims=True)  # (the VALUE: which zero's sign it carries is not promised)
    return np.broadcast_to(m, x.shape).reshape(v.shape), np.broadcast_to(ok.any(axis=2, keepdims=True), x.shape).reshape(v.shape)


def wave_sum_tree(v):
    """the tree wave_sum_f64's comment states: xor 1, 2, 4, 8 inside each row of 16 lanes, then (r0 + r1) + (r2 + r3); every lane"""
    v = np.array(v, dtype=np.float64)
    for off in (1, 2, 4, 8):
        v = v + v[:, LANES ^ off]
    s = (v[:, 0] + v[:, 16]) + (v[:, 32] + v[:, 48])
    return np.repeat(s[:, None], 64, axis=1)


def reference(name, in0, in1=None):
    """(words [nrows x 64] u64, mask [nrows x 64] bool) -- what each lane must hold after the call, and where that is fixed by the contract"""
    in0 = np.ascontiguousarray(in0, dtype=np.uint64)
    full = np.ones(in0.shape, dtype=bool)
    with np.errstate(all="ignore"):
        if name in MIN_F64:
            m, ok = _grouped_min_f64(_f64(in0), MIN_F64[name])
            return _bits(m).reshape(in0.shape), ok
        if name == "PDMP_WAVE_SCAN_MIN_F64":
            v = _f64(in0)
            ok = ~np.isnan(v)
            return _bits(np.minimum.accumulate(np.where(ok, v, INF), axis=1)).reshape(in0.shape), np.logical_or.accumulate(ok, axis=1)
        if name in MIN_U32:
            g = MIN_U32[name]
            u = (in0 & np.uint64(0xFFFFFFFF)).reshape(len(in0), 64 // g, g)
            return np.ascontiguousarray(np.broadcast_to(u.min(axis=2, keepdims=True), u.shape).reshape(in0.shape)), full
        if name == "PDMP_WAVE_SCAN_ADD_U32":
            return np.cumsum(in0 & np.uint64(0xFFFFFFFF), axis=1, dtype=np.uint64) & np.uint64(0xFFFFFFFF), full
        if name == "PDMP_WAVE_BPERM_F64":
            src = np.ascontiguousarray(in1, dtype=np.uint64).astype(np.int64)
            assert ((src >= 0) & (src < 64)).all()
            return np.take_along_axis(in0, src, axis=1), full
        assert name == "PDMP_WAVE_SUM_F64", name
        return _bits(wave_sum_tree(_f64(in0))).reshape(in0.shape), full


def same(name, dev, ref):
    """bit for bit -- except a zero minimum, whose sign is outside the contract (min(+0, -0) may return either operand)"""
    dev = np.ascontiguousarray(dev, dtype=np.uint64)
    eq = dev == ref
    if name in MIN_F64 or name == "PDMP_WAVE_SCAN_MIN_F64":
        eq |= (_f64(ref) == 0.0) & (_f64(dev) == 0.0)
    return eq
