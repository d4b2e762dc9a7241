"""The references of the callback and random-stream tests, checked on the CPU before anything on the device is held
against them: tests/philox_ref.py against the published Philox4x32-10 known answers, tests/keras_callbacks_ref.py
against the two other restatements of SURVEY.md A.5 in this repository."""
import numpy as np
import pytest

from oracle import locator_oracle as O
from tests import keras_callbacks_ref as KR
from tests import philox_ref as PR

# Random123 known answers (kat_vectors, philox4x32 with 10 rounds): counter words, key words -> output words
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_reference_reproduces_the_known_answers():
    for ctr, key, out in KNOWN_ANSWERS:
        assert PR.philox4x32_10_words(ctr, key).tolist() == list(out)
        # the 64-bit form packs the words little end first
        lo, hi, k = ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32, key[0] | key[1] << 32
        assert PR.philox(lo, hi, k).tolist() == list(out)
    # vectorised over counters = one call per counter, and a stream slice = the slice of the stream
    lo = np.array([0, 1, (1 << 32) + 5, (1 << 64) - 1], dtype=np.uint64)
    both = PR.philox(lo, 0x6d61736b, 0x123456789abcdef0)
    for i, c in enumerate(lo.tolist()):
        assert both[i].tolist() == PR.philox(c, 0x6d61736b, 0x123456789abcdef0).tolist()
    whole = PR.stream_words(0, 64, 7, 9)
    assert whole.dtype == np.uint32 and PR.stream_words(8, 11, 7, 9).tolist() == whole[8:19].tolist()


def test_value_maps_are_fp32_step_by_step():
    r = np.array([0, 1, 0x7fffffff, 0x80000000, 0xffffff7f, 0xffffff80, 0xffffffff], dtype=np.uint32)
    u = PR.u01(r)
    assert u.dtype == np.float32
    # 0 -> 2^-33; from 2^24 on the conversion rounds to nearest even, and the top of the range reaches 1.0 exactly
    assert u[0] == np.float32(2.0 ** -33) and u[-1] == np.float32(1.0) and u[4] < 1.0 and u[5] == np.float32(1.0)
    v = PR.uniform_pm(r, 0.25)
    assert v.dtype == np.float32 and v[0] == np.float32(-0.25) and v[-1] == np.float32(0.25)
    assert PR.glorot_limit(2, 1) == np.float32(np.sqrt(2.0)) and PR.glorot_limit(70, 40).dtype == np.float32
    assert PR.dropout_threshold(0.0) == 0 and PR.dropout_threshold(0.25) == 1 << 30 and PR.dropout_threshold(0.5) == 1 << 31
    assert PR.dropout_threshold(0.1) % 256 != 0
    m = PR.dropout_mask_ref(4096, 0.0, 3, 0)
    assert m.dtype == np.uint8 and m.all()
    assert abs(float(PR.dropout_mask_ref(1 << 16, 0.25, 3, 4).mean()) - 0.75) < 0.01


@pytest.mark.parametrize("name", sorted(KR.SEQUENCES))
def test_three_restatements_of_the_callbacks_agree(name):
    """tests/keras_callbacks_ref.py, oracle.Callbacks and locator_amd.train.Callbacks, epoch by epoch: save, stop, the
    logged LR and every piece of state.  oracle.Callbacks has lr_patience = int(patience / 6) and factor 0.5 built in,
    so it takes part where the sequence's parameters are those."""
    from locator_amd.train import Callbacks as TrainCallbacks
    vals, patience, lr_patience, factor = KR.SEQUENCES[name]
    ref = KR.KerasCallbacks(patience, lr_patience, factor, KR.LR0)
    others = {"train": TrainCallbacks(patience, KR.LR0, lr_patience, factor)}
    if lr_patience == int(patience / 6) and factor == 0.5:
        others["oracle"] = O.Callbacks(patience, KR.LR0)
    for epoch, v in enumerate(vals):
        save, stop, logged, _ = ref.on_epoch_end(epoch, np.float64(v))
        want = (save, stop, float(logged), ref.ck.best, ref.es.best, ref.es.wait, ref.rl.best, ref.rl.wait, float(ref.rl.lr))
        for who, cb in others.items():
            s, t, l = cb.on_epoch_end(epoch, float(v))
            got = (bool(s), bool(t), float(l), cb.ck_best, cb.es_best, cb.es_wait, cb.rl_best, cb.rl_wait, float(cb.lr))
            assert got == want, (name, who, epoch, got, want)


def test_device_trace_freezes_after_the_stop():
    vals, patience, lr_patience, factor = KR.SEQUENCES["main-p6-lp1-f0.5"]
    tr = KR.device_trace(vals, patience, lr_patience, factor, KR.LR0)
    stop = next(e for e, s in enumerate(tr) if s["stopped"])
    assert stop == 23 and len(vals) - 1 - stop >= 3 and tr[stop]["row"][2] in (2.0, 6.0)
    frozen = {k: v for k, v in tr[stop].items() if k not in ("epoch", "save_now", "row")}
    for e in range(stop + 1, len(vals)):
        assert {k: tr[e][k] for k in frozen} == frozen and tr[e]["row"] is None and tr[e]["save_now"] == 0
        assert tr[e]["epoch"] == e + 1
    # the plateau of epochs 12-15 is long enough for two reductions at lr_patience 2, and the LR stays a normal number
    tr2 = KR.device_trace(*KR.SEQUENCES["main-p12-lp2-f0.25"], KR.LR0)
    assert [e for e in range(12, 16) if tr2[e]["row"][2] >= 4] == [13, 15] and tr2[29]["stopped"] and not tr2[28]["stopped"]
    for name, (vals, p, lp, f) in KR.SEQUENCES.items():
        lrs = [float(s["lr"]) for s in KR.device_trace(vals, p, lp, f, KR.LR0)]
        assert min(lrs) > 1.2e-38 and lrs[-1] >= KR.LR0 * 0.25 ** 60, name
