"""Edge tables and plain references of the queue helpers probed by pdmp_debug_queue_eval / pdmp_debug_state_eval (include/pdmp_debug.h:
PDMP_QUEUE_*, PDMP_STATE_*): the lossy first-level codes of the one-proposal-per-lane kernels (p_* of pdmp_trackp.hip: 8 ulp margin, 3 position
bits; q_* of pdmp_exactp.hip: 16 ulp, 4 bits), the nine-bit wheel of pdmp_trackl.hip, pdmp_below, the neighbour-id tests and the two exact
first levels.

The references are numpy restatements (astype(float32) is round-to-nearest-even); the claims about exact values -- "a lower bound", "at most 2
ulps below" -- are checked with fractions.Fraction in tests/test_wave_queue_tables_ref.py (on the references) and in
tests/test_gpu_queue_codes.py (on what the device returned).
"""
from fractions import Fraction

import numpy as np

IDS = {"PDMP_QUEUE_P_ENC": 0, "PDMP_QUEUE_P_THR": 1, "PDMP_QUEUE_P_DEC": 2, "PDMP_QUEUE_Q_ENC": 3, "PDMP_QUEUE_Q_THR": 4, "PDMP_QUEUE_Q_DEC": 5,
       "PDMP_QUEUE_TL_Q": 6, "PDMP_QUEUE_BELOW": 7, "PDMP_QUEUE_HB": 8, "PDMP_QUEUE_NB_HAS": 9, "PDMP_QUEUE_NB_COUNT": 10}
STATE_WHEEL, STATE_LEVEL1, STATE_S8_LEVEL1 = 0, 1, 2


class Code:
    """one family of first-level codes: `bits` position bits, the nearest float's pattern lowered by `margin` before they are cleared"""

    def __init__(self, prefix, bits, margin, infbits):
        self.prefix, self.nbits, self.mask, self.margin, self.infbits = prefix, bits, (1 << bits) - 1, margin, infbits
        self.enc_id, self.thr_id, self.dec_id = (IDS["PDMP_QUEUE_%s_%s" % (prefix, s)] for s in ("ENC", "THR", "DEC"))


CODES = {"P": Code("P", 3, 8, 0x7F7FFFF8), "Q": Code("Q", 4, 16, 0x7F7FFFF0)}

INF = np.inf
DENORM_MIN = 5e-324
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN_NORMAL = 2.0**-126
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN_NORMAL = 2.0**-1022
BASES = (0.0, 0.75, -3.5, 1e6, 12345.678)


def up(x):
    with np.errstate(over="ignore"):  # (above DBL_MAX lies +Inf)
        return np.nextafter(x, INF)


def down(x):
    with np.errstate(over="ignore"):
        return np.nextafter(x, -INF)


def around(x):
    return [float(down(x)), float(x), float(up(x))]


# ------------------------------------------------------------------------------------------------ the codes: tables

def float_midpoints():
    """[(lower float, midpoint, upper float, does the tie go up)]: exact midpoints between adjacent floats in several binades, ties both ways"""
    out = []
    for e in (-140, -127, -126, -60, -20, -10, -1, 0, 1, 6, 23, 24, 60, 127):
        for k in (0, 1, 2, 5, (1 << 23) - 2, (1 << 23) - 1):
            if e == 127 and k == (1 << 23) - 1:
                continue  # (above FLT_MAX there is no float: that midpoint is in differences() by itself)
            if e < -126:  # subnormal floats: multiples of 2^-149
                f1 = (2.0 ** (e + 149) + k % 4) * 2.0**-149
                f2 = f1 + 2.0**-149
            else:
                f1 = 2.0**e * (1 + k * 2.0**-23)
                f2 = 2.0**e * (1 + (k + 1) * 2.0**-23)
            assert np.float32(f1) == f1 and np.float32(f2) == f2 and np.nextafter(np.float32(f1), np.float32(INF)) == np.float32(f2)
            mid = (f1 + f2) / 2  # exact: one more bit than a float has
            assert Fraction(mid) * 2 == Fraction(f1) + Fraction(f2)
            goes_up = bool(np.float32(f1).view(np.uint32) & 1)  # ties to even: up iff the lower float's pattern is odd
            out.append((f1, mid, f2, goes_up))
    return out


def differences():
    """key - tb, as doubles"""
    rng = np.random.default_rng(0xD1FF)
    d = [0.0, -1.0, -1e-300, -DENORM_MIN, -1e6, DENORM_MIN, 2 * DENORM_MIN, 1e-300]
    d += around(2.0**-149) + around(2.0**-150) + around(2.0**-126) + around(2.0**-125)
    for _, mid, _, _ in float_midpoints():
        d += around(mid)
    d += [1e-3, 0.25, float(up(0.25)), 1.0, 100.0]
    d += list(rng.uniform(0.0, 100.0, 300))
    d += [2.0**24 + 1, 2.0**24 + 3] + around(FLT_MAX)
    d += around(2.0**128 - 2.0**103)  # the midpoint between FLT_MAX and 2^128: from here on the nearest float is +Inf
    d += [2.0**128, 1e39, 1e300, DBL_MAX, INF]
    return np.array(d)


def key_rows():
    """(key, tb) for every base and difference: key = tb + difference as a double (what the difference then IS follows from the pair)"""
    d = differences()
    with np.errstate(over="ignore"):
        return (np.concatenate([tb + d for tb in BASES]), np.concatenate([np.full(len(d), tb) for tb in BASES]))


def enc_rows(code):
    """(key, tb, pos): every position value for every (key, tb)"""
    key, tb = key_rows()
    npos = code.mask + 1
    return np.repeat(key, npos), np.repeat(tb, npos), np.tile(np.arange(npos, dtype=np.float64), len(key))


def thr_rows():
    """(tau, tb, key): tau equal to the key and to its double neighbours on either side"""
    key, tb = key_rows()
    key, tb = key[np.isfinite(key)], tb[np.isfinite(key)]
    return np.concatenate([down(key), key, up(key)]), np.tile(tb, 3), np.tile(key, 3)


# ------------------------------------------------------------------------------------------------ the codes: references

def f32_pattern(dlt):
    """bit pattern of the nearest float (ties to even) of max(dlt, 0); a NaN counts as 0 like in `(dlt > 0.0) ? dlt : 0.0`"""
    with np.errstate(all="ignore"):
        dlt = np.where(dlt > 0.0, dlt, 0.0)
        return dlt.astype(np.float32).view(np.uint32).astype(np.int64)


def nearest_is_subnormal(key, tb):
    """the nearest float of the difference is subnormal: whether the conversion keeps or flushes it is the device's choice"""
    b = f32_pattern(np.asarray(key) - np.asarray(tb))
    return (b > 0) & (b < 0x00800000)


def enc_ref(code, key, tb, pos):
    with np.errstate(all="ignore"):
        b = f32_pattern(np.asarray(key, dtype=np.float64) - np.asarray(tb, dtype=np.float64))
    return (np.where(b >= code.margin, b - code.margin, 0) & ~np.int64(code.mask)) | np.asarray(pos).astype(np.int64)


def thr_ref(code, tau, tb):
    """the nearest float's pattern + 1, and never below the patterns a block AT the base carries (its position bits)"""
    with np.errstate(all="ignore"):
        b = f32_pattern(np.asarray(tau, dtype=np.float64) - np.asarray(tb, dtype=np.float64))
    return np.maximum(b + 1, code.mask)


def pattern_float(code, bits):
    """the float a pattern stands for (position bits cleared), as a double"""
    return (np.asarray(bits).astype(np.int64) & ~np.int64(code.mask)).astype(np.uint32).view(np.float32).astype(np.float64)


def dec_ref(code, bits, tb):
    with np.errstate(all="ignore"):
        return down(np.asarray(tb, dtype=np.float64) + pattern_float(code, bits))


def nearest_f32_pattern_exact(x):
    """pattern of the float nearest to the non-negative Fraction x (ties to even), 0x7f800000 beyond the last midpoint: no double rounding"""
    if x >= Fraction(2) ** 128 - Fraction(2) ** 103:
        return 0x7F800000
    g = float(x)  # within one double rounding of x: the answer is one of the floats around it
    with np.errstate(over="ignore"):
        c = min(int(np.float32(g).view(np.uint32)), 0x7F7FFFFF)
    best = None
    for p in (c - 1, c, c + 1):
        if 0 <= p <= 0x7F7FFFFF:
            err = abs(Fraction(float(np.uint32(p).view(np.float32))) - x)
            if best is None or err < best[0] or (err == best[0] and p % 2 == 0):
                best = (err, p)
    return best[1]


# ------------------------------------------------------------------------------------------------ the codes: invariants
# What the comments of p_enc / p_thr / p_dec (and q_*) promise, as checks on ANY implementation's outputs over the tables above: the reference's
# (tests/test_wave_queue_tables_ref.py) and the device's (tests/test_gpu_queue_codes.py).  Where the nearest float of the difference is
# subnormal the conversion may keep or flush it; (a) to (d) hold either way, tightness (e) is claimed for the other rows only.

def _fr(x):
    return Fraction(float(x))


def _pat_fr(m):
    return Fraction(float(np.uint32(m).view(np.float32)))


def check_enc(c, key, tb, pos, enc):
    """(a) position bits, (b) exact lower bound, (c) monotone, (e) tightness, (f) the +Inf patterns -- of enc [len(key)] for enc_rows(c)"""
    enc = np.asarray(enc).astype(np.int64)
    assert ((enc & c.mask) == np.asarray(pos).astype(np.int64)).all(), "(a) the low bits are the position"
    masked = enc & ~np.int64(c.mask)
    sub = nearest_is_subnormal(key, tb)
    n_inf = n_tight = 0
    seen = {}
    for k, t, m, sb in zip(key, tb, masked, sub):
        if (k, t) in seen:
            assert seen[(k, t)] == m, ("the pattern does not depend on the position", k, t)
            continue
        seen[(k, t)] = m
        if not k >= t:
            assert m == 0, ("a key below the base counts as the base", k, t, m)
            continue
        diff = None if k == INF else _fr(k) - _fr(t)
        near = 0x7F800000 if diff is None else nearest_f32_pattern_exact(diff)
        if near == 0x7F800000:
            assert m >= c.infbits, ("(f) +Inf, or a difference whose nearest float is +Inf", k, t, m)
            n_inf += 1
            continue
        if diff <= _fr(FLT_MAX):
            assert m < c.infbits, ("(f) a finite difference at or below FLT_MAX", k, t, m)
        if m < c.infbits:
            assert _pat_fr(m) <= diff, ("(b) the decoded float is a lower bound of key - tb", k, t, m)
        assert m <= near, ("(b)", k, t, m, near)
        if not sb:
            assert near - (c.margin + c.mask) <= m, ("(e) at most margin + mask patterns below the nearest float's", k, t, m, near)
            n_tight += 1
    for base in BASES:
        sel = np.asarray(tb) == base
        o = np.argsort(np.asarray(key)[sel], kind="stable")
        assert (np.diff(masked[sel][o]) >= 0).all(), ("(c) monotone in the key", base)
    return n_inf, n_tight


def check_thr(c, tau, tb, key, thr, top):
    """(d) key <= tau implies enc(key, tb, pos) <= thr(tau, tb) for every pos -- top is enc with the largest position -- and thr is monotone"""
    thr, top = np.asarray(thr).astype(np.int64), np.asarray(top).astype(np.int64)
    le = key <= tau
    bad = le & (top > thr)
    assert not bad.any(), ("(d)", list(zip(key[bad][:4], tau[bad][:4], tb[bad][:4], top[bad][:4], thr[bad][:4])))
    for base in BASES:
        sel = tb == base
        o = np.argsort(tau[sel], kind="stable")
        assert (np.diff(thr[sel][o]) >= 0).all(), ("thr is monotone in tau", base)
    return int(le.sum())


def check_dec(c, key, tb, bits, dec):
    """(b) dec(enc(key), tb) <= key as doubles wherever key >= tb; (e) at most 2 double ulps below the exact tb + float, and never above it"""
    bits = np.asarray(bits).astype(np.int64)
    finite = (bits & ~np.int64(c.mask)) < c.infbits
    ge = (key >= tb) & finite
    assert (dec[ge] <= key[ge]).all(), ("(b)", key[ge][dec[ge] > key[ge]][:4])
    n = 0
    for t, m, dv in zip(tb[::c.mask + 1], bits[::c.mask + 1] & ~np.int64(c.mask), dec[::c.mask + 1]):
        if m < c.infbits:
            exact = _fr(t) + _pat_fr(m)
            assert _fr(dv) <= exact <= _fr(up(up(dv))), ("(e) one rounding, then one step down", t, m, dv)
            n += 1
    return n


def pattern_is_normal_or_zero(c, bits):
    m = np.asarray(bits).astype(np.int64) & ~np.int64(c.mask)
    return (m == 0) | (m >= 0x00800000)


# ------------------------------------------------------------------------------------------------ tl_q, pdmp_below, hb_*, nb_*

TLQ_TOP, TLQ_BOTTOM = 2147483520.0, -2147483648.0  # the two saturation limits


def tlq_columns():
    """[(t sorted ascending, tref, s)]: exact integer products and their neighbours, both saturation limits and theirs, +-Inf, tiny and huge s"""
    cols = []
    vs = [0.0, 0.5, 1.0, 2.0, 3.0, 1000.0, 2.0**24, TLQ_TOP - 128, TLQ_TOP - 1, TLQ_TOP, TLQ_TOP + 1, 2147483647.0, 2.0**31, 2.0**31 + 1000, 2.0**40, 1e300]
    vs += [-v for v in vs] + [TLQ_BOTTOM + 1, TLQ_BOTTOM + 0.5, TLQ_BOTTOM - 1]
    for tref, s in ((0.0, 1.0), (0.75, 4.0), (-3.5, 1024.0), (0.0, 30.0), (1e6, 1e-3), (12345.678, 1e9), (0.0, 1e-300), (0.75, 1e300), (0.0, 2.0**-1074),
                    (-3.5, DBL_MAX)):
        with np.errstate(all="ignore"):
            t = np.array([x for v in vs for x in around(tref + v / s)] + [-INF, INF, tref] + around(tref))
        t = np.unique(t[~np.isnan(t)])
        cols.append((t, tref, s))
    return cols


def tlq_rows():
    cols = tlq_columns()
    return (np.concatenate([t for t, _, _ in cols]), np.concatenate([np.full(len(t), r) for t, r, _ in cols]),
            np.concatenate([np.full(len(t), s) for t, _, s in cols]))


def tlq_ref(t, tref, s):
    with np.errstate(all="ignore"):
        v = np.floor((np.asarray(t) - tref) * s)
    assert not np.isnan(v).any()  # (a NaN's conversion is outside the contract: the table has none)
    return np.where(v >= TLQ_TOP, 2.0**31 - 1, np.where(v <= TLQ_BOTTOM, -(2.0**31), v))


def below_inputs():
    rng = np.random.default_rng(0xBE10)
    x = [0.0, -0.0, DENORM_MIN, -DENORM_MIN, 1.0, -1.0, DBL_MAX, -DBL_MAX, DBL_MIN_NORMAL, -DBL_MIN_NORMAL, INF, 2.0, -2.0, 0.5, 1e-310, -1e-310]
    return np.concatenate([x, rng.standard_normal(64) * 2.0 ** rng.integers(-1000, 1000, 64)])


def hb_ref(b):
    """(word, bit mask) of block b's ninth bit, from the layout the comment states: b = 16 (o + 64 j) + 4 w + y is byte y of word w of the
    16-byte piece j of lane o; its bit is 8 y + w + 4 (j & 1) of word 4 o + (j >> 1)"""
    b = np.asarray(b, dtype=np.int64)
    y, w, o, j = b & 3, (b >> 2) & 3, (b >> 4) & 63, b >> 10
    return 4 * o + (j >> 1), np.int64(1) << (8 * y + w + 4 * (j & 1))


def nb_rows():
    """(a, b, v, ids): the eight 16-bit halves of a uint4 as the bit images of two doubles (0 to 8 ids, 0xFFFF fillers at the end) and a value"""
    rng = np.random.default_rng(0x1D5)
    rows = []
    for n in range(9):
        for rep in range(4):
            ids = list(rng.choice(1 << 15, n, replace=False))
            if n and rep == 0:
                ids[0] = 0
            if n and rep == 1:
                ids[-1] = (1 << 15) - 1
            if n >= 2 and rep == 2:
                ids[0], ids[1] = (1 << 15) - 1, 0
            ids = [int(i) for i in ids]
            vs = list(ids)  # present, in each of the halves in turn
            vs += [i ^ (1 << k) for i in ids[:2] for k in range(15)]  # one bit away from a present id
            vs += [0, 1, (1 << 15) - 1, (1 << 15) - 2] + [int(q) for q in rng.integers(0, 1 << 15, 4)]
            for v in vs:
                rows.append((ids, v))
    a = np.empty(len(rows), dtype=np.uint64)
    b = np.empty(len(rows), dtype=np.uint64)
    for k, (ids, _) in enumerate(rows):
        h = ids + [0xFFFF] * (8 - len(ids))
        a[k] = h[0] | (h[1] << 16) | (h[2] << 32) | (h[3] << 48)
        b[k] = h[4] | (h[5] << 16) | (h[6] << 32) | (h[7] << 48)
    return a.view(np.float64), b.view(np.float64), np.array([v for _, v in rows], dtype=np.float64), [ids for ids, _ in rows]


# ------------------------------------------------------------------------------------------------ the wheel's images

NB2 = 8192


def wheel_writes():
    """[(b, w9)] in order; among them second writes to the same b that flip the ninth bit both ways, and neighbours inside one word of the bit plane"""
    rng = np.random.default_rng(0x9B17)
    w = [(0, 0x1FF), (1, 0x100), (15, 0x0FF), (16, 0x1AB), (1023, 0x155), (1024, 0x0AA), (2047, 0x101), (2048, 0x1FE), (8191, 0x1FF)]
    w += [(int(b), int(v)) for b, v in zip(rng.integers(0, NB2, 300), rng.integers(0, 512, 300))]
    w += [(16, 0x0AB), (1024, 0x1AA), (8191, 0x0FF), (0, 0x0FF), (0, 0x1FF)]  # ninth bit off again, on again, and off then on
    for b in (4000, 4001, 4002, 4003, 4000 + 1024, 4000 + 2048):  # (word 4 o + (b >> 11): b and b + 1024 share it, b + 2048 has the next)
        w += [(b, 0x1C3)]
    w += [(4001, 0x0C3), (4000 + 1024, 0x03C)]  # clearing one bit leaves its neighbours in the word alone
    return w


def wheel_ref(writes):
    img = {}
    for b, w9 in writes:
        img[b] = w9
    return np.array([img.get(b, 0) for b in range(NB2)], dtype=np.float64)  # (never written: the cleared value)


# ------------------------------------------------------------------------------------------------ the exact first levels

def level1_state(keys, block, d=None, nout=None):
    """(bk, bi): the minimum of every block of `block` keys and the lowest index attaining it, of the keys as they stand; the refresh clock's slot d
    is no coordinate (+Inf whatever it holds); entries past the last block are (+Inf, 0)"""
    k = np.array(keys, dtype=np.float64)
    if d is not None:
        k[d] = INF
    k = k.reshape(-1, block)
    bk, bi = k.min(axis=1), k.argmin(axis=1) + block * np.arange(len(k))  # (argmin: the first of equal minima)
    if nout is not None:
        bk = np.concatenate([bk, np.full(nout - len(bk), INF)])
        bi = np.concatenate([bi, np.zeros(nout - len(bi), dtype=bi.dtype)])
    return bk, bi.astype(np.float64)


def level1_ref(keys, changes, block, d=None, nout=None):
    """([4 x nout], [nchg x 2]): the first level after the build and after the changes, and the changed block's entry after each change.  An update leaves an entry alone when the changed key neither undercuts
    it nor was it -- which keeps a right entry right -- so the state after every change is again the one of the keys as they stand."""
    k = np.array(keys, dtype=np.float64)
    bk0, bi0 = level1_state(k, block, d, nout)
    steps = []  # the entry of the changed key's block right after each update
    for j, kj in changes:
        k[j] = kj
        bk, bi = level1_state(k, block, d)
        steps.append((bk[j // block], bi[j // block]))
    bk1, bi1 = level1_state(k, block, d, nout)
    return np.vstack([bk0, bi0, bk1, bi1]), np.array(steps)


def level1_case(nblk, block, refresh=False):
    """(keys, changes, d or None): random finite keys with ties inside blocks and (from two blocks on) one whole block of +Inf; the changes hold a key
    that rises while it was the entry (the rescan), ties from a lower and from a higher index, an undercut, a change that touches nothing, and
    the +Inf block coming alive and going back"""
    rng = np.random.default_rng(1000 * block + nblk)
    n = nblk * block
    keys = rng.uniform(1.0, 2.0, n)
    if nblk >= 2:
        keys[block:2 * block] = INF
    d = None
    if refresh:  # d is no multiple of the block: the clock's slot lies inside the last block, the keys behind it are padding
        d = n - block + block // 2 + 3
        keys[d + 1:] = INF
        keys[d] = 0.001  # (the clock's time, smaller than every key: it must not become the entry)
    last = (d if refresh else n) - 1  # the last coordinate
    keys[5], keys[14] = 0.5, 0.5       # a tie inside block 0: the lower index is the entry
    ch = []
    ch.append((5, 3.0))                # the entry of block 0 rises: rescan, the other 0.5 at 14 takes over
    ch.append((7, 0.5))                # ties the entry (14) from a lower index: replaces it
    ch.append((15, 0.5))               # ties the entry (7) from a higher index: nothing
    ch.append((9, 0.25))               # undercuts
    ch.append((11, 2.5))               # neither: nothing
    ch.append((9, 0.75))               # the entry rises above the tied 0.5s: rescan finds 7, the lowest of them
    if nblk >= 2:
        ch.append((block + 4, 1.25))   # the +Inf block comes alive
        ch.append((block + 9, 1.25))   # a tie from a higher index: nothing
        ch.append((block + 4, INF))    # ... its entry leaves: rescan finds the other
        ch.append((block + 9, INF))    # ... and the block is +Inf again: (+Inf, first index)
    ch.append((last, 0.125))           # the last coordinate undercuts its block (beside the parked clock where there is one)
    ch.append((last, 4.0))             # ... and rises again: the rescan must not see the clock's slot
    for _ in range(40):                # random changes, now and then of the entry itself
        j = int(rng.integers(0, last + 1))
        if rng.random() < 0.3:
            bk, bi = level1_state(_apply(keys, ch), block, d)
            j = int(bi[rng.integers(0, len(bi))])
            if d is not None and j >= d:
                j = last
        ch.append((j, float(rng.choice([0.5, 0.75, 1.5, INF, rng.uniform(0.1, 3.0)]))))
    return keys, ch, d


def _apply(keys, changes):
    k = np.array(keys)
    for j, kj in changes:
        k[j] = kj
    return k


LEVEL1_CASES = [(nblk, 64, False) for nblk in (1, 2, 3, 65)] + [(nblk, 32, r) for nblk in (1, 2, 3, 65) for r in (False, True)]
