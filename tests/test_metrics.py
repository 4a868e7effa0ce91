"""The device accumulator (``pa_eval_*``, csrc/metrics.hip) on seeded random log-probabilities against numpy.

Integers (rows, correct, ignored, bad_labels, the whole confusion matrix) must be exact. The two double sums are held to the
textbook bound of a sum of n terms in ANY order, ``n * 2**-53 * sum|term|`` (the kernel's order is a per-wave walk, a fixed
tree per workgroup and an ordered slab; the reference is ``math.fsum``), plus for ``conf_sum`` one ulp for each side's ``exp``:
``(n + 4) * 2**-52 * sum(term)``."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTIONS = (1, 2, 63, 64, 65, 200)          # below, at and above one wave, more than one column per lane
ROWS = (0, 1, 63, 64, 65, 257, 4099)       # nothing, one row, a partial wave / workgroup, several slab partials, more rows than slab slots x waves
PAD_VALUE = np.float32(3.0e38)             # what sits in the columns >= A of a wide row: it would win every argmax if it were read


def _case(A, ld, n, seed, dirty):
    """-> (logp float32[n, ld], labels int32[n]): log_softmax of normal noise, rows 0 / 1 with the maximum duplicated at
    several / at all A positions, labels cycling through hit, miss, ignored, random and (dirty) out of range."""
    g = torch.Generator().manual_seed(seed)
    logp = torch.full((n, ld), float(PAD_VALUE), dtype=torch.float32)
    logp[:, :A] = torch.log_softmax(torch.randn((n, A), generator=g, dtype=torch.float32) * 2.0, dim=1)
    if n >= 1 and A >= 2:
        pos = [A - 1, A // 3] + ([A // 3 + 64] if A // 3 + 64 < A - 1 else [])   # other lanes, and the same lane one stride on
        logp[0, pos] = logp[0, :A].max() + 1.0
    if n >= 2:
        logp[1, :A] = -math.log(A)
    lp = logp.numpy()
    pred = lp[:, :A].argmax(axis=1)
    rng = np.random.default_rng(seed + 1)
    labels = rng.integers(0, A, n).astype(np.int32)
    r = np.arange(n)
    labels[r % 5 == 0] = pred[r % 5 == 0]
    labels[r % 5 == 1] = (pred[r % 5 == 1] + 1) % A
    labels[r % 5 == 2] = -100
    if dirty:
        bad = np.array([A, -1, A + 1000, -101, np.iinfo(np.int32).min], dtype=np.int64)
        labels[r % 5 == 4] = bad[(r[r % 5 == 4] // 5) % len(bad)].astype(np.int32)
    return logp, labels


def _expected(lp, labels, A):
    pred = lp[:, :A].argmax(axis=1)
    ignored = labels == -100
    bad = ~ignored & ((labels < 0) | (labels >= A))
    ok = ~ignored & ~bad
    y, p = labels[ok].astype(np.int64), pred[ok]
    cm = np.zeros((A, A), dtype=np.int64)
    np.add.at(cm, (y, p), 1)
    nll_terms = -lp[ok, y].astype(np.float64)
    conf_terms = np.exp(lp[ok, p].astype(np.float64))
    return dict(rows=int(ok.sum()), correct=int((y == p).sum()), ignored=int(ignored.sum()), bad_labels=int(bad.sum()), cm=cm,
                nll=math.fsum(nll_terms), nll_abs=math.fsum(np.abs(nll_terms)), conf=math.fsum(conf_terms), pred=pred)


def _check(totals, cm, want, where):
    n = want["rows"]
    nll_err, conf_err = abs(totals["nll_sum"] - want["nll"]), abs(totals["conf_sum"] - want["conf"])
    nll_bar, conf_bar = n * 2.0 ** -53 * want["nll_abs"], (n + 4) * 2.0 ** -52 * want["conf"]
    print(f"{where}: rows={n} nll_err={nll_err:.3e} (bar {nll_bar:.3e}) conf_err={conf_err:.3e} (bar {conf_bar:.3e})")
    for k in ("rows", "correct", "ignored", "bad_labels"):
        assert totals[k] == want[k], (where, k, totals[k], want[k])
    assert np.array_equal(cm, want["cm"]), where
    assert nll_err <= nll_bar, (where, totals["nll_sum"], want["nll"])
    assert conf_err <= conf_bar, (where, totals["conf_sum"], want["conf"])


def _read(es, dirty):
    """-> (totals dict, confusion); a dirty case must come back as PA_ERR_BAD_LABELS with everything filled in."""
    from playaid_core_amd import _lib, metrics

    if not dirty:
        t, cm = es.totals()
        return metrics._totals_dict(t), cm
    raw = _lib.pa_eval_totals()
    assert es._lib.pa_eval_read(es._h, ctypes.byref(raw), None, es._stream()) == _lib.PA_ERR_BAD_LABELS   # the matrix is optional
    with pytest.raises(metrics.BadLabelsError) as info:
        es.totals()
    assert info.value.totals == metrics._totals_dict(raw) and info.value.totals["bad_labels"] > 0
    t, cm = es.totals(strict=False)
    assert metrics._totals_dict(t) == info.value.totals and np.array_equal(cm, info.value.confusion)
    return info.value.totals, cm


@pytest.mark.parametrize("A", ACTIONS)
def test_accumulator_matches_numpy(A):
    from playaid_core_amd.metrics import EvalState

    dev = torch.device("cuda:0")
    with EvalState(A, dev) as es:
        for ld in (A, A + 3):
            for n in ROWS:
                for dirty in (False, True):
                    if dirty and n < 5:
                        continue   # (no row of such a case takes an out-of-range label)
                    logp, labels = _case(A, ld, n, seed=1000 * A + 10 * n + ld, dirty=dirty)
                    want = _expected(logp.numpy(), labels, A)
                    assert (want["bad_labels"] > 0) == dirty
                    ld_dev, lab_dev = logp.to(dev), torch.from_numpy(labels).to(dev)
                    if n:   # the kernel's prediction is torch.argmax's on the same tensor (first index on ties)
                        assert np.array_equal(torch.argmax(ld_dev[:, :A], dim=1).cpu().numpy(), want["pred"])
                    es.reset()
                    es.update(ld_dev, lab_dev)
                    totals, cm = _read(es, dirty)
                    _check(totals, cm, want, f"A={A} ld={ld} n={n} dirty={dirty}")
                    if n >= 2 and A >= 2:   # rows 0 and 1 carry the duplicated maxima: their predictions are the first index
                        assert want["pred"][0] == A // 3 and want["pred"][1] == 0
                    if n == 65:
                        # a records-shaped label source: int32[n, 4] with the label in field 1 (pa_record.action_id), stride 4
                        rec = torch.full((n, 4), 1 << 20, dtype=torch.int32)
                        rec[:, 1] = torch.from_numpy(labels)
                        es.reset()
                        es.update(ld_dev, rec.to(dev).view(-1)[1:], label_stride=4)
                        t2, cm2 = _read(es, dirty)
                        assert t2 == totals and np.array_equal(cm2, cm)   # same rows in the same order: the same bits
                        # ... and a narrow view of a wide tensor takes its pitch from the stride
                        if ld > A:
                            es.reset()
                            es.update(ld_dev[:, :A], lab_dev)
                            t3, cm3 = _read(es, dirty)
                            assert t3 == totals and np.array_equal(cm3, cm)


def _bits(t):
    return struct.pack("<dd", t["nll_sum"], t["conf_sum"])


@pytest.mark.parametrize("A", (63, 200))
def test_state_persists_across_calls_and_is_deterministic(A):
    from playaid_core_amd.metrics import EvalState

    dev = torch.device("cuda:0")
    n = 4099
    logp, labels = _case(A, A, n, seed=77 + A, dirty=False)
    want = _expected(logp.numpy(), labels, A)
    ld_dev, lab_dev = logp.to(dev), torch.from_numpy(labels).to(dev)
    cuts = (0, 1000, 3000, n)
    with EvalState(A, dev) as es:
        es.update(ld_dev, lab_dev)
        whole, whole_cm = _read(es, False)
        runs = []
        for _ in range(2):
            es.reset()
            for a, b in zip(cuts[:-1], cuts[1:]):
                es.update(ld_dev[a:b], lab_dev[a:b])
            es.update(ld_dev[:0], lab_dev[:0])   # n == 0: a no-op
            runs.append(_read(es, False))
        for i, (t, cm) in enumerate(runs):
            _check(t, cm, want, f"A={A} split run {i}")
            assert {k: t[k] for k in ("rows", "correct", "ignored", "bad_labels")} == {k: whole[k] for k in ("rows", "correct", "ignored", "bad_labels")}
            assert np.array_equal(cm, whole_cm)
        assert _bits(runs[0][0]) == _bits(runs[1][0])   # the same calls in the same order: the same bits
        # and the one-call form twice
        es.reset()
        es.update(ld_dev, lab_dev)
        again, _ = _read(es, False)
        assert _bits(again) == _bits(whole)
        # without a reset the state keeps adding: twice the integers
        es.update(ld_dev, lab_dev)
        twice, cm2 = _read(es, False)
        assert twice["rows"] == 2 * whole["rows"] and twice["correct"] == 2 * whole["correct"] and np.array_equal(cm2, 2 * whole_cm)
        assert abs(twice["nll_sum"] - 2 * want["nll"]) <= 2 * want["rows"] * 2.0 ** -53 * 2 * want["nll_abs"]


def test_update_refuses_tensors_it_cannot_score():
    from playaid_core_amd.metrics import EvalState

    dev = torch.device("cuda:0")
    with EvalState(5, dev) as es:
        logp = torch.zeros((4, 5), device=dev)
        lab = torch.zeros(4, dtype=torch.int32, device=dev)
        for bad_logp, bad_lab, stride in ((logp[:, :4], lab, 1), (logp.double(), lab, 1), (logp.cpu(), lab, 1), (logp, lab.long(), 1),
                                          (logp, lab[:3], 1), (logp, lab, 2), (logp, lab, 0), (torch.zeros((5, 4), device=dev).t(), lab, 1)):
            with pytest.raises(ValueError):
                es.update(bad_logp, bad_lab, stride)
        t, cm = es.totals()
        assert t.rows == 0 and t.ignored == 0 and not cm.any()   # nothing of the above reached the device
