"""The 64-lane primitives every event loop rests on, each CALLED by a probe kernel of the unit that owns it (pdmp_debug_wave_eval /
pdmp_debug_state_eval, parity library) on the edge tables of wave_tables.py / queue_tables.py and held to the plain references there (-m gpu).

A failure names the helper: a wrong DPP control, row mask or bank mask shows in the one-hot rows of its own id instead of as "events differ"
after 10^5 events of a chain."""
import numpy as np
import pytest

import queue_tables as Q
import wave_tables as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(W.IDS, key=W.IDS.get))
def test_wave_primitive_matches_its_reference(gpu_pkg_parity, name):
    """Bit for bit the reference in every lane the function's comment promises: every lane for the uniform forms (wave_min_*, wave_sum_f64), for
    the group / row forms and for the scans; bperm_f64 for source lanes 0 .. 63.  Two things are asserted as a PROPERTY, not as bits: the sign
    of a zero minimum (min(+0, -0) may return either operand), and a minimum over lanes some of which hold a quiet NaN -- it equals the
    minimum of the non-NaN lanes ("NaN loses"); a group or prefix of NaN lanes only is left out.
    Seen on an MI355X: the minimum over lanes that hold both zeros came back as -0 in every lane of every f64 form (v_min_f64 orders -0
    below +0), and every promised lane of the rows with quiet-NaN lanes held the minimum of the other lanes bit for bit."""
    in0, in1 = W.tables(name)
    dev = gpu_pkg_parity._lib.wave_eval(W.IDS[name], in0, in1)
    ref, mask = W.reference(name, in0, in1)
    ok = W.same(name, dev, ref) | ~mask
    if name in W.MIN_F64 or name == "PDMP_WAVE_SCAN_MIN_F64":  # (what the device did where only the property is asserted)
        v, r, dv = in0.view(np.float64), ref.view(np.float64), dev.view(np.float64)
        z = mask & (r == 0.0) & (dv == 0.0) & (np.signbit(v) != np.signbit(v[:, :1])).any(axis=1, keepdims=True)
        nanrow = mask & np.isnan(v).any(axis=1, keepdims=True)
        print("%s: a zero minimum of a row holding both zeros came back as -0 in %d lanes, as +0 in %d; lanes of rows with NaN equal to the reference "
              "bit for bit: %d of %d" % (name, int(np.signbit(dv[z]).sum()), int((~np.signbit(dv[z])).sum()), int((dev == ref)[nanrow].sum()), int(nanrow.sum())))
    bad = np.argwhere(~ok)
    assert ok.all(), (name, len(bad), [(int(r), int(l), hex(int(dev[r, l])), hex(int(ref[r, l]))) for r, l in bad[:6]],
                      "row %d: %s" % (bad[0][0], [hex(int(x)) for x in in0[bad[0][0]]]))


@pytest.mark.parametrize("nblk,block,refresh", Q.LEVEL1_CASES)
def test_level1_build_and_update(gpu_pkg_parity, nblk, block, refresh):
    """level1_build / level1_update (blocks of 64) and s8_build_level1 / s8_level1_update (blocks of 32, the refresh clock's slot parked inside
    the last block): every entry is (the block's minimum, the lowest index attaining it) of the keys as they stand, after the build and after a
    list of changes that holds a rescan, ties from a lower and from a higher index, an undercut, and a whole block of +Inf -- and the entry of the
    changed key's block is that right after every single update."""
    keys, ch, d = Q.level1_case(nblk, block, refresh)
    fn = Q.STATE_LEVEL1 if block == 64 else Q.STATE_S8_LEVEL1
    dev, dev_steps = gpu_pkg_parity._lib.state_eval(fn, keys, ch, d=(d if refresh else len(keys)), has_refresh=refresh)
    ref, ref_steps = Q.level1_ref(keys, ch, block, d, 512 if block == 32 else None)
    assert dev.shape == ref.shape and dev_steps.shape == ref_steps.shape
    bad = np.flatnonzero((dev_steps != ref_steps).any(axis=1))  # the changed block's entry right after every single update
    assert len(bad) == 0, [(int(k), ch[k], tuple(dev_steps[k]), tuple(ref_steps[k])) for k in bad[:6]]
    for row, what in enumerate(("minima after the build", "indices after the build", "minima after the changes", "indices after the changes")):
        bad = np.flatnonzero(dev[row] != ref[row])
        assert len(bad) == 0, (what, [(int(b), dev[row, b], ref[row, b]) for b in bad[:6]])


def test_wheel_images_round_trip(gpu_pkg_parity):
    """img_set / img_get of pdmp_trackl.hip: after the write list (second writes to one block flip the ninth bit both ways, neighbours share a
    word of the bit plane) img_get of all 8192 blocks equals a dictionary model; cells never written read as the cleared value"""
    w = Q.wheel_writes()
    dev = gpu_pkg_parity._lib.state_eval(Q.STATE_WHEEL, None, w)
    ref = Q.wheel_ref(w)
    bad = np.flatnonzero(dev != ref)
    assert len(bad) == 0, [(int(b), dev[b], ref[b]) for b in bad[:8]]


def test_state_probe_refuses_an_index_outside_its_array(gpu_pkg_parity):
    """every probe index stays inside its buffer: the host refuses the list before any kernel runs"""
    L = gpu_pkg_parity._lib
    for fn, keys, ch in ((Q.STATE_WHEEL, None, [(8192, 1.0)]), (Q.STATE_WHEEL, None, [(0, 512.0)]), (Q.STATE_LEVEL1, np.ones(64), [(64, 1.0)]),
                         (Q.STATE_S8_LEVEL1, np.ones(32), [(32, 1.0)])):
        with pytest.raises(L.PdmpError) as ei:
            L.state_eval(fn, keys, ch, d=(0 if keys is None else len(keys)))
        assert ei.value.code == L.PDMP_ERR_INVALID
