"""The tracked queues' first-level codes and their relatives, each CALLED by a probe kernel of the unit that owns it (pdmp_debug_queue_eval,
parity library) on the edge tables of queue_tables.py (-m gpu): p_enc / p_thr / p_dec of pdmp_trackp.hip, q_* of pdmp_exactp.hip, the
wheel's tl_q and hb_word / hb_bit of pdmp_trackl.hip, pdmp_below, nb_has / nb_count.

The codes are lossy on purpose; what must never fail is stated by their comments -- a bound that is stale LOW, never high; a threshold that is
the largest pattern a block with exact minimum <= tau can carry; monotone in the key -- and is asserted here on the device's own outputs in
exact rational arithmetic (queue_tables.check_*), next to bit-for-bit equality with the numpy restatement."""
import numpy as np
import pytest

import queue_tables as Q

pytestmark = pytest.mark.gpu


def _mismatch(dev, ref, sel, *cols):
    bad = np.flatnonzero(sel & (dev != ref))
    return len(bad), [tuple(float(c[k]) for c in cols) + (float(dev[k]), float(ref[k])) for k in bad[:6]]


@pytest.mark.parametrize("name", [n for n in sorted(Q.IDS, key=Q.IDS.get) if n.endswith(("_ENC", "_THR", "_DEC"))])
def test_first_level_code(gpu_pkg_parity, name):
    """p_* (mask 7, margin 8) and q_* (mask 15, margin 16) over every base, difference and position of the table:
    (a) the low bits equal pos; (b) a finite pattern's float is <= key - tb exactly whenever key >= tb, and dec(enc(key), tb) <= key;
    (c) key1 <= key2 orders the masked patterns; (d) key <= tau implies enc(key, tb, pos) <= thr(tau, tb) for every pos; (e) the masked
    pattern lies at most margin + mask (15 / 31) patterns below the nearest float's, dec at most 2 double ulps below the exact tb + float;
    (f) +Inf and differences whose nearest float is +Inf give a pattern >= INFBITS, no difference at or below FLT_MAX does; (g) bit for bit
    the numpy restatement wherever the nearest float of the difference is normal or zero.
    Where the nearest float is SUBNORMAL only (a) to (d) are asserted: the conversion may keep or flush it.  Seen on an MI355X under this build's
    flags: v_cvt_f32_f64 KEEPS subnormal results (all 320 such rows of p_enc and 640 of q_enc equal the numpy restatement bit for bit), and
    p_dec / q_dec read every subnormal pattern back as the same subnormal (408 / 816 rows).
    (d) is what showed the one fault this test found: the table rows with key = tau = tb (difference 0, every base) and pos >= 2 -- a block AT
    the base carries its bare position bits, up to 7 / 15, above the former threshold `pattern + 1` = 1; p_thr / q_thr now never return less than
    the mask."""
    L = gpu_pkg_parity._lib
    c = Q.CODES[name.split("_")[2]]
    key, tb, pos = Q.enc_rows(c)
    enc = L.queue_eval(c.enc_id, key, tb, pos)[0]
    assert (enc == np.floor(enc)).all() and enc.min() >= 0 and enc.max() < 2.0**32
    if name.endswith("_ENC"):
        ref = Q.enc_ref(c, key, tb, pos)
        sub = Q.nearest_is_subnormal(key, tb)
        n, ex = _mismatch(enc, ref, ~sub, key, tb, pos)
        assert n == 0, ("(g)", n, ex)
        print("%s: %d of %d rows whose nearest float is subnormal equal the numpy restatement (subnormals kept); %d differ from it and read 0 + pos (flushed)"
              % (name, int((enc == ref)[sub].sum()), int(sub.sum()), int(((enc == pos) & (enc != ref))[sub].sum())))
        n_inf, n_tight = Q.check_enc(c, key, tb, pos, enc)
        assert n_inf >= 20 and n_tight >= 1500
    elif name.endswith("_THR"):
        tau, ttb, tkey = Q.thr_rows()
        thr = L.queue_eval(c.thr_id, tau, ttb)[0]
        top = L.queue_eval(c.enc_id, tkey, ttb, np.full(len(tkey), float(c.mask)))[0]  # (the device's own patterns, largest position)
        assert Q.check_thr(c, tau, ttb, tkey, thr, top) >= 2 * len(tkey) // 3
        n, ex = _mismatch(thr, Q.thr_ref(c, tau, ttb), ~Q.nearest_is_subnormal(tau, ttb), tau, ttb)
        assert n == 0, ("(g)", n, ex)
    else:
        dec = L.queue_eval(c.dec_id, enc, tb)[0]  # of the device's own patterns
        assert Q.check_dec(c, key, tb, enc, dec) >= 1500
        ref = Q.dec_ref(c, enc, tb)
        normal = Q.pattern_is_normal_or_zero(c, enc)
        same = (dec.view(np.uint64) == ref.view(np.uint64))
        assert same[normal].all(), ("(g)", int((~same[normal]).sum()), list(zip(enc[normal & ~same][:6], tb[normal & ~same][:6], dec[normal & ~same][:6])))
        print("%s: %d of %d subnormal patterns decode like the numpy restatement (read back as subnormals)" % (name, int(same[~normal].sum()), int((~normal).sum())))


def test_tl_q(gpu_pkg_parity):
    """the quantum of a time: bit for bit the numpy restatement floor((t - tref) s) saturated at 2147483520 / -2^31 (exact integer products and
    their neighbours, both limits and theirs, +-Inf, tiny and huge s; no NaN), and monotone along every sorted column of the table"""
    t, tref, s = Q.tlq_rows()
    dev = gpu_pkg_parity._lib.queue_eval(Q.IDS["PDMP_QUEUE_TL_Q"], t, tref, s)[0]
    n, ex = _mismatch(dev, Q.tlq_ref(t, tref, s), np.ones(len(t), dtype=bool), t, tref, s)
    assert n == 0, (n, ex)
    k = 0
    for col, _, _ in Q.tlq_columns():
        assert (np.diff(dev[k:k + len(col)]) >= 0).all()
        k += len(col)


def test_pdmp_below(gpu_pkg_parity):
    """the largest double below x: np.nextafter(x, -inf) on +-0, +-denorm_min, +-1, +-DBL_MAX, the smallest normal, +Inf and random values"""
    x = Q.below_inputs()
    dev = gpu_pkg_parity._lib.queue_eval(Q.IDS["PDMP_QUEUE_BELOW"], x)[0]
    ref = Q.down(x)
    same = dev.view(np.uint64) == ref.view(np.uint64)
    assert same.all(), list(zip(x[~same], dev[~same], ref[~same]))


def test_hb_word_and_bit(gpu_pkg_parity):
    """the place of a block's ninth bit: over b = 0 .. 8191 the pairs (word, bit) are 8192 distinct places in 256 words of 32 bits, and the 128
    blocks lane o = (b >> 4) & 63 scans map exactly onto words 4 o .. 4 o + 3 ("a lane's 128 blocks are its own 16 bytes"); equal to the
    layout the comment states (queue_tables.hb_ref)"""
    b = np.arange(Q.NB2)
    dev = gpu_pkg_parity._lib.queue_eval(Q.IDS["PDMP_QUEUE_HB"], b.astype(np.float64))
    word, bit = dev[0].astype(np.int64), dev[1].astype(np.int64)
    assert (word == dev[0]).all() and (bit == dev[1]).all() and word.min() >= 0 and word.max() < 256
    assert all(0 < m < (1 << 32) and m & (m - 1) == 0 for m in bit.tolist())
    assert len(set(zip(word.tolist(), bit.tolist()))) == Q.NB2
    o = (b >> 4) & 63
    for lane in range(64):
        assert set(word[o == lane].tolist()) == {4 * lane, 4 * lane + 1, 4 * lane + 2, 4 * lane + 3}
    rw, rb = Q.hb_ref(b)
    assert (word == rw).all() and (bit == rb).all(), np.flatnonzero((word != rw) | (bit != rb))[:8]


@pytest.mark.parametrize("name", ["PDMP_QUEUE_NB_HAS", "PDMP_QUEUE_NB_COUNT"])
def test_neighbour_ids(gpu_pkg_parity, name):
    """nb_has is set membership among the eight 16-bit halves and nb_count the number of ids before the 0xFFFF fillers: 0 to 8 ids, id 0,
    id 2^15 - 1, v in each of the eight halves, v absent but one bit away from a present id"""
    a, b, v, ids = Q.nb_rows()
    dev = gpu_pkg_parity._lib.queue_eval(Q.IDS[name], a, b, v)[0]
    ref = np.array([float(int(x) in i) for x, i in zip(v, ids)]) if name.endswith("HAS") else np.array([float(len(i)) for i in ids])
    bad = np.flatnonzero(dev != ref)
    assert len(bad) == 0, [(ids[k], int(v[k]), dev[k], ref[k]) for k in bad[:6]]
