"""The references of tests/wave_tables.py and tests/queue_tables.py satisfy, on every table row, the invariants the GPU tests hold the device to
(tests/test_gpu_wave_primitives.py, tests/test_gpu_queue_codes.py): the tables are known good before a device sees them.  No GPU needed.

Each reference is checked here against a SECOND, slower statement of the same contract -- plain Python loops over lanes, Python integers,
fractions.Fraction for the claims about exact values -- and the tables against the list of edges they are there to reach."""
from fractions import Fraction

import numpy as np
import pytest

import oracle_lib as O
import queue_tables as Q
import wave_tables as W


def f64(w):
    return np.ascontiguousarray(w, dtype=np.uint64).view(np.float64)


# ------------------------------------------------------------------------------------------------ wave primitives

@pytest.mark.parametrize("name", sorted(W.MIN_F64))
def test_min_f64_reference_and_table(name):
    g = W.MIN_F64[name]
    t, _ = W.tables(name)
    ref, mask = W.reference(name, t)
    v, r = f64(t), f64(ref)
    nan = np.isnan(v)
    assert (t[nan] == W.QNAN).all() and nan.any() and not nan.all(axis=1).any()  # quiet NaN only, beside finite lanes; no all-NaN row
    for row in range(len(t)):
        for g0 in range(0, 64, g):
            lanes = [x for x in v[row, g0:g0 + g] if x == x]
            if not lanes:
                assert not mask[row, g0:g0 + g].any()  # a group of NaN lanes only: left out
                continue
            assert mask[row, g0:g0 + g].all()
            m = r[row, g0]
            assert (r[row, g0:g0 + g] == m).all() and all(m <= x for x in lanes) and any(m == x for x in lanes)  # the minimum of the non-NaN lanes, in every lane
    # the edges: the strict minimum in every lane L (one-hot), ties, +Inf everywhere and with one finite lane, denormals, mixed zeros
    clean = ~nan.any(axis=1)
    strict = [(v[k] == v[k].min()).sum() == 1 and clean[k] for k in range(len(v))]
    assert {int(v[k].argmin()) for k in range(len(v)) if strict[k]} == set(range(64))
    assert any((v[k] == v[k].min()).sum() > 1 and v[k].min() < v[k].max() for k in range(len(v)) if clean[k])
    assert (v == np.inf).all(axis=1).any() and {int(np.isfinite(x).argmax()) for x in v if np.isfinite(x).sum() == 1 and (x[~np.isfinite(x)] == np.inf).all()} == set(range(64))
    assert ((v != 0) & (np.abs(v) < 2.0**-1022)).any() and (v == W.DENORM_MIN).any()
    assert any((x == 0).all() and len(set(np.signbit(x))) == 2 for x in v)
    assert (np.diff(v, axis=1) < 0).all(axis=1).any() and (np.diff(v, axis=1) > 0).all(axis=1).any()


def test_scan_min_f64_reference_and_table():
    t, _ = W.tables("PDMP_WAVE_SCAN_MIN_F64")
    ref, mask = W.reference("PDMP_WAVE_SCAN_MIN_F64", t)
    v, r = f64(t), f64(ref)
    for row in range(len(t)):
        run, seen = np.inf, False
        for lane in range(64):
            x = v[row, lane]
            if x == x:
                run, seen = min(run, x), True
            assert bool(mask[row, lane]) == seen  # (a prefix of NaN lanes only: left out)
            if seen:
                assert r[row, lane] == run
    for k in W.PREFIXES:  # rows whose first k lanes hold the identity
        assert any((x[:k] == np.inf).all() and np.isfinite(x[k:]).all() for x in v), k


@pytest.mark.parametrize("name", sorted(W.MIN_U32))
def test_min_u32_reference_and_table(name):
    g = W.MIN_U32[name]
    t, _ = W.tables(name)
    ref, mask = W.reference(name, t)
    assert mask.all() and (t < (1 << 32)).all()
    for row in range(len(t)):
        for g0 in range(0, 64, g):
            assert (ref[row, g0:g0 + g] == min(int(x) for x in t[row, g0:g0 + g])).all()
    strict = [(x == x.min()).sum() == 1 for x in t]
    assert {int(x.argmin()) for x, s in zip(t, strict) if s} == set(range(64))  # the minimum in the one lane a wrong DPP control skips
    assert (t == 0xFFFFFFFF).all(axis=1).any()
    assert any(((x == 0xFFFFFFFF).sum() == 63) for x in t)  # one-hot against 0xffffffff
    assert any(x.min() < (1 << 31) <= x.max() and (x >= (1 << 31)).sum() > 32 for x in t)  # both sides of 2^31


def test_scan_add_u32_reference_and_table():
    t, _ = W.tables("PDMP_WAVE_SCAN_ADD_U32")
    ref, mask = W.reference("PDMP_WAVE_SCAN_ADD_U32", t)
    assert mask.all()
    wraps = 0
    for row in range(len(t)):
        s = 0
        for lane in range(64):
            s += int(t[row, lane])
            assert int(ref[row, lane]) == s % (1 << 32)
        wraps += s >= (1 << 32)
    assert wraps >= 10 and any(int(x.astype(object).sum()) == 1 << 32 for x in t)  # rows that wrap past 2^32, one of them exactly onto 0
    for k in W.PREFIXES:
        assert any((x[:k] == 0).all() and (x[k:] > 0).all() for x in t), k


def test_bperm_reference_and_table():
    val, src = W.tables("PDMP_WAVE_BPERM_F64")
    ref, mask = W.reference("PDMP_WAVE_BPERM_F64", val, src)
    assert mask.all() and (src < 64).all()  # a source lane is 0 .. 63: nothing else is documented
    for row in range(len(val)):
        for lane in range(64):
            assert ref[row, lane] == val[row, int(src[row, lane])]
    assert any((s == np.arange(64)).all() for s in src) and any(len(set(s)) == 1 for s in src) and any(sorted(s) == list(range(64)) and (s != np.arange(64)).all() for s in src)


def test_wave_sum_reference_is_the_stated_tree_and_the_oracles_order():
    """wave_sum_f64's comment: xor 1, 2, 4, 8, then (r0 + r1) + (r2 + r3).  The numpy restatement equals the oracle's dot_wave64 (its xor
    butterfly 1 .. 32 ends in the same grouping) on every row, and the heavy-cancellation rows tell it from other orders of the same additions."""
    t, _ = W.tables("PDMP_WAVE_SUM_F64")
    ref, mask = W.reference("PDMP_WAVE_SUM_F64", t)
    v, r = f64(t), f64(ref)
    assert mask.all() and np.isfinite(v).all() and (r == r[:, :1]).all()
    ones = np.ones(64)
    for row in range(len(v)):
        a = np.ascontiguousarray(v[row])
        orc = O.lib().orc_dot_wave64(a.ctypes.data, ones.ctypes.data, 64)
        assert orc == r[row, 0], (row, orc, r[row, 0])  # (the oracle starts every lane's partial sum from +0: equal as values)
    seq = np.array([sum(float(x) for x in row) for row in v])  # lane 0 + lane 1 + ... in order
    rs = _row_sums(v)
    flat = ((rs[:, 0] + rs[:, 1]) + rs[:, 2]) + rs[:, 3]  # the rows of 16 the same way, then ((r0 + r1) + r2) + r3
    assert (seq != r[:, 0]).sum() >= 20 and (flat != r[:, 0]).sum() >= 5


def _row_sums(v):
    """the four sums over the rows of 16 lanes as the tree forms them (xor 1, 2, 4, 8)"""
    v = np.array(v)
    for off in (1, 2, 4, 8):
        v = v + v[:, W.LANES ^ off]
    return v[:, [0, 16, 32, 48]]


# ------------------------------------------------------------------------------------------------ the first-level codes

@pytest.mark.parametrize("code", sorted(Q.CODES))
def test_code_references_satisfy_the_invariants(code):
    """(a) to (f) of the codes' contract (queue_tables.check_*), on the numpy restatement over every table row"""
    c = Q.CODES[code]
    key, tb, pos = Q.enc_rows(c)
    assert set(pos) == set(range(c.mask + 1))  # every position value
    enc = Q.enc_ref(c, key, tb, pos)
    n_inf, n_tight = Q.check_enc(c, key, tb, pos, enc)
    assert n_inf >= 20 and n_tight >= 1500
    assert Q.check_dec(c, key, tb, enc, Q.dec_ref(c, enc, tb)) >= 1500
    tau, ttb, tkey = Q.thr_rows()
    thr = Q.thr_ref(c, tau, ttb)
    assert Q.check_thr(c, tau, ttb, tkey, thr, Q.enc_ref(c, tkey, ttb, np.full(len(tkey), c.mask))) >= 2 * len(tkey) // 3
    assert (thr[np.isfinite(tau) & (tau - ttb <= Q.FLT_MAX)] <= 0x7F800000).all()
    # "always 0" passes (a) to (d) and must fail (e); a bound one pattern too high must fail (b)
    with pytest.raises(AssertionError):
        Q.check_enc(c, key, tb, pos, pos.astype(np.int64))
    with pytest.raises(AssertionError):
        Q.check_enc(c, key, tb, pos, enc + (c.margin + c.mask + 1 if c.prefix == "P" else 2 * c.margin))


def test_code_table_reaches_the_edges():
    key, tb = Q.key_rows()
    d0 = key[tb == 0.0]  # (with base 0 the difference is the key itself)
    for x in (0.0, Q.DENORM_MIN, 2.0**-149, 2.0**-126, 1e-3, 2.0**24 + 1, Q.FLT_MAX, np.inf):
        assert x in d0, x
    assert (key < tb).any() and ((key == tb).sum() >= len(Q.BASES))  # negative differences; a key equal to the base, for every base
    ups = downs = 0
    for f1, mid, f2, goes_up in Q.float_midpoints():  # exact midpoints, both ties-to-even directions, and their double neighbours on either side
        assert {float(Q.down(mid)), mid, float(Q.up(mid))} <= set(d0)
        got = np.float32(mid)
        assert got == (f2 if goes_up else f1) and np.float32(Q.down(mid)) == f1 and np.float32(Q.up(mid)) == f2
        ups, downs = ups + goes_up, downs + (not goes_up)
    assert ups >= 10 and downs >= 10
    assert Q.nearest_is_subnormal(key, tb).any()
    r = d0[(d0 > 0) & (d0 < 100)]
    assert len(r) >= 300
    # a midpoint reached from a base other than 0: key = 0.75 + midpoint is exact
    assert any(Fraction(float(k)) - Fraction(0.75) == Fraction(m) for k in key[tb == 0.75] for _, m, _, _ in Q.float_midpoints()[40:50])


# ------------------------------------------------------------------------------------------------ the other queue helpers

def test_tlq_reference_is_monotone_and_saturates():
    hit_top = hit_bottom = exact = 0
    for t, tref, s in Q.tlq_columns():
        q = Q.tlq_ref(t, tref, s)
        assert (np.diff(t) > 0).all() and (np.diff(q) >= 0).all()  # monotone along every sorted column
        assert (q == np.floor(q)).all() and q.min() >= -(2.0**31) and q.max() <= 2.0**31 - 1
        assert q[0] == -(2.0**31) and q[-1] == 2.0**31 - 1  # -Inf and +Inf
        hit_top += int((q == 2.0**31 - 1).sum())
        hit_bottom += int((q == -(2.0**31)).sum())
        with np.errstate(all="ignore"):
            v = (t - tref) * s
        exact += int(((v == np.floor(v)) & (np.abs(v) < 2.0**31) & (v != 0)).sum())
        for lim in (Q.TLQ_TOP, Q.TLQ_BOTTOM):  # the limit itself and a product just inside it
            if 1e-3 <= s <= 1e9 and tref == 0.0:
                assert (v == lim).any()
        if s == 1.0 and tref == 0.0:
            assert Q.tlq_ref(np.array([2147483519.0]), 0.0, 1.0)[0] == 2147483519.0 and Q.tlq_ref(np.array([2147483520.0]), 0.0, 1.0)[0] == 2.0**31 - 1
            assert Q.tlq_ref(np.array([-2147483647.5]), 0.0, 1.0)[0] == -(2.0**31) and Q.tlq_ref(np.array([-2147483647.0]), 0.0, 1.0)[0] == -2147483647.0
    assert hit_top >= 20 and hit_bottom >= 20 and exact >= 40
    assert not np.isnan(Q.tlq_rows()[0]).any()


def test_below_table():
    x = Q.below_inputs()
    for v in (0.0, Q.DENORM_MIN, -Q.DENORM_MIN, 1.0, -1.0, Q.DBL_MAX, -Q.DBL_MAX, Q.DBL_MIN_NORMAL, np.inf):
        assert v in x
    assert any(v == 0 and np.signbit(v) for v in x) and not np.isnan(x).any() and not (x == -np.inf).any()
    y = Q.down(x)
    assert (y < x).all() and y[list(x).index(0.0)] == -Q.DENORM_MIN and y[list(x).index(np.inf)] == Q.DBL_MAX and y[list(x).index(-Q.DBL_MAX)] == -np.inf


def test_ids_are_the_headers():
    """the ids the tables send are the ones include/pdmp_debug.h defines"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pdmp_debug.h")).read()
    ids = {m[0]: int(m[1]) for m in re.findall(r"#define (PDMP_(?:WAVE|QUEUE|STATE)_\w+) (\d+)", src)}
    assert {k: v for k, v in ids.items() if k.startswith("PDMP_WAVE_")} == W.IDS
    assert {k: v for k, v in ids.items() if k.startswith("PDMP_QUEUE_")} == Q.IDS
    assert (ids["PDMP_STATE_WHEEL"], ids["PDMP_STATE_LEVEL1"], ids["PDMP_STATE_S8_LEVEL1"]) == (Q.STATE_WHEEL, Q.STATE_LEVEL1, Q.STATE_S8_LEVEL1)


def test_hb_layout_reference():
    b = np.arange(Q.NB2)
    word, bit = Q.hb_ref(b)
    assert word.min() == 0 and word.max() == 255 and all(int(m).bit_length() <= 32 and bin(int(m)).count("1") == 1 for m in bit)
    assert len({(int(w), int(m)) for w, m in zip(word, bit)}) == Q.NB2  # 8192 distinct places in 256 words of 32 bits
    for o in range(64):  # the 128 blocks lane o scans are exactly the bits of words 4 o .. 4 o + 3: its own 16 bytes
        mine = ((b >> 4) & 63) == o
        assert mine.sum() == 128 and set(word[mine]) == {4 * o, 4 * o + 1, 4 * o + 2, 4 * o + 3}
        assert not np.isin(word[~mine], [4 * o, 4 * o + 1, 4 * o + 2, 4 * o + 3]).any()


def test_wheel_write_list_and_model():
    w = Q.wheel_writes()
    img = Q.wheel_ref(w)
    assert all(0 <= b < Q.NB2 and 0 <= v < 512 for b, v in w)
    seen, on_off, off_on = {}, 0, 0
    for b, v in w:
        if b in seen:
            on_off += (seen[b] & 256) and not (v & 256)
            off_on += (not (seen[b] & 256)) and bool(v & 256)
        seen[b] = v
    assert on_off >= 2 and off_on >= 2  # second writes to the same b flip the ninth bit both ways
    assert all(img[b] == v for b, v in seen.items()) and (img[[b for b in range(Q.NB2) if b not in seen]] == 0).all() and len(seen) < Q.NB2 // 2
    words = {}
    for b in seen:
        words.setdefault(int(Q.hb_ref(b)[0]), []).append(b)
    assert any(len(v) >= 3 for v in words.values())  # several written blocks share a word of the bit plane


def test_nb_table():
    a, b, v, ids = Q.nb_rows()
    halves = np.stack([(a.view(np.uint64) >> np.uint64(16 * h)) & np.uint64(0xFFFF) for h in range(4)]
                      + [(b.view(np.uint64) >> np.uint64(16 * h)) & np.uint64(0xFFFF) for h in range(4)], axis=1)
    where = set()
    for k in range(len(v)):
        n = len(ids[k])
        assert list(halves[k, :n]) == ids[k] and (halves[k, n:] == 0xFFFF).all() and all(0 <= i < (1 << 15) for i in ids[k]) and 0 <= v[k] < (1 << 15)
        if v[k] in ids[k]:
            where.add(ids[k].index(int(v[k])))
    assert {len(i) for i in ids} == set(range(9)) and where == set(range(8))  # 0 to 8 ids; v present in each of the eight halves
    assert any(0 in i for i in ids) and any((1 << 15) - 1 in i for i in ids)
    near = [k for k in range(len(v)) if int(v[k]) not in ids[k] and any(bin(int(v[k]) ^ i).count("1") == 1 for i in ids[k])]
    assert len(near) >= 100  # absent, but one bit away from a present id


# ------------------------------------------------------------------------------------------------ the exact first levels

def _replay(keys, changes, block, d, drop=None):
    """the update rule as the header states it: a smaller key (or an equal one at a lower index) replaces the entry; the entry's own key growing
    rescans the block; anything else leaves the entry alone.  Returns the state and which rule each change took."""
    k = np.array(keys, dtype=np.float64)
    bk, bi = Q.level1_state(k, block, d)
    took, steps = [], []
    for j, kj in changes:
        k[j] = kj
        b = j // block
        if drop:  # a WRONG rule, to show that the per-change entries tell it from the right one
            if kj < bk[b] or (drop != "tie" and kj == bk[b] and j < bi[b]):
                bk[b], bi[b] = kj, j
            elif bi[b] == j and drop != "rescan":
                nb, ni = Q.level1_state(k, block, d)
                bk[b], bi[b] = nb[b], ni[b]
            steps.append((bk[b], bi[b]))
            continue
        if kj < bk[b] or (kj == bk[b] and j < bi[b]):
            took.append("tie_lower" if kj == bk[b] else "undercut")
            bk[b], bi[b] = kj, j
        elif bi[b] == j:
            took.append("rescan")
            nb, ni = Q.level1_state(k, block, d)
            bk[b], bi[b] = nb[b], ni[b]
        else:
            took.append("tie_higher" if kj == bk[b] else "nothing")
        full = Q.level1_state(k, block, d)
        assert (bk == full[0]).all() and (bi == full[1]).all(), (j, kj)  # leaving a right entry alone keeps it right
    return np.array(steps) if drop else (bk, bi, took)


@pytest.mark.parametrize("nblk,block,refresh", Q.LEVEL1_CASES)
def test_level1_reference_and_cases(nblk, block, refresh):
    keys, ch, d = Q.level1_case(nblk, block, refresh)
    assert len(keys) == nblk * block and all(0 <= j < len(keys) and j != d for j, _ in ch)
    ref, steps = Q.level1_ref(keys, ch, block, d, 512 if block == 32 else None)
    bk, bi, took = _replay(keys, ch, block, d)
    assert steps.shape == (len(ch), 2) and all(steps[k][0] <= kj and (steps[k][1] == j or steps[k][0] < kj or steps[k][1] < j) for k, (j, kj) in enumerate(ch))
    for rule in ("tie", "rescan"):  # an update rule without its tie clause, or without its rescan, shows in the per-change entries of every case
        assert (_replay(keys, ch, block, d, drop=rule) != steps).any(), rule
    assert (ref[2, :nblk] == bk).all() and (ref[3, :nblk] == bi).all()
    assert {"rescan", "tie_lower", "tie_higher", "undercut", "nothing"} <= set(took)
    k = np.array(keys)
    for row, kk in ((0, k), (2, Q._apply(keys, ch))):
        if d is not None:
            kk = kk.copy()
            kk[d] = np.inf
        for b in range(nblk):
            blk = kk[b * block:(b + 1) * block]
            assert ref[row, b] == blk.min() and ref[row + 1, b] == b * block + list(blk).index(blk.min())  # the minimum, the lowest index attaining it
    if block == 32:
        assert (ref[[0, 2], nblk:] == np.inf).all() and (ref[[1, 3], nblk:] == 0).all()
    if nblk >= 2:
        assert (k[block:2 * block][np.arange(block) + block != (d if d is not None else -1)] == np.inf).all() and ref[0, 1] == np.inf and ref[1, 1] == block
    if refresh:  # the parked slot: inside the last block, not at its start, smaller than every key, and never the entry
        assert d % 32 != 0 and d // 32 == nblk - 1 and k[d] < np.delete(k, d).min() and d not in ref[[1, 3]]
