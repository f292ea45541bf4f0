"""CPU checks of the sparse per-query-mask plumbing (filter_query_masks_sparse): which groups
the planner marks `qmask` in sparse mode under each of its conditions, that the dense rule is
untouched, the config knob, and armi_sparse_topk_qmask's argument errors (no device work)."""

import pytest


def _plan(filters, sizes=None, knob=0, n_rows=10000, **kw):
    from audio_rag_amd.retrieval.mi355x import plan_filter_groups

    kw.setdefault("mode", "sparse")
    kw.setdefault("sparse_masks", True)
    return plan_filter_groups(filters, n_rows, knob, lambda f: (sizes or {})[f["a"]], **kw)


BROAD = [{"a": 1}, None, {"a": 2}, {"a": 1}, {}, None]


def test_sparse_mode_marks_every_masked_group_the_unfiltered_one_included():
    groups = _plan(BROAD)
    assert [(g.filter, g.queries, g.rowlist, g.qmask) for g in groups] == [
        ({"a": 1}, [0, 3], False, True), (None, [1, 4, 5], False, True),
        ({"a": 2}, [2], False, True)]


@pytest.mark.parametrize("kw", [
    {"sparse_masks": False},                    # the knob
    {"tail_rows": 1},                           # a live tail: armi_sparse_tail_topk takes one mask
], ids=["knob", "tail"])
def test_sparse_mode_conditions(kw):
    assert all(not g.qmask for g in _plan(BROAD, **kw))
    assert all(g.qmask for g in _plan(BROAD))


def test_sparse_mode_default_is_off():
    from audio_rag_amd.retrieval.mi355x import plan_filter_groups

    for kw in ({}, {"query_masks": True, "qmask_supported": lambda n: True}):
        groups = plan_filter_groups(BROAD, 10000, 0, lambda f: 0, mode="sparse", **kw)
        assert all(not g.qmask and not g.rowlist for g in groups)


@pytest.mark.parametrize("kw", [
    {"query_masks": False}, {"query_masks": True},
    {"query_masks": True, "qmask_supported": lambda n: False},
    {"query_masks": True, "qmask_supported": lambda n: True},
    {"qmask_supported": None},
], ids=["dense-off", "dense-on", "unsupported", "supported", "no-index-answer"])
def test_sparse_mode_ignores_the_dense_knob_and_the_dense_index(kw):
    assert all(g.qmask for g in _plan(BROAD, **kw))


def test_sparse_mode_never_asks_the_dense_index():
    def supported(n):
        raise AssertionError("the sparse form has no shape limit")

    assert all(g.qmask for g in _plan(BROAD, qmask_supported=supported))
    assert all(g.qmask for g in _plan([{"a": i % 3} for i in range(300)],
                                      qmask_supported=supported))


@pytest.mark.parametrize("mode", ["dense", "legacy_dense", "hybrid"])
def test_the_sparse_knob_marks_nothing_in_the_other_modes(mode):
    assert all(not g.qmask for g in _plan(BROAD, mode=mode))
    # and changes nothing there when the dense rule applies
    kw = {"mode": mode, "query_masks": True, "qmask_supported": lambda n: True}
    on = _plan(BROAD, sparse_masks=True, **kw)
    off = _plan(BROAD, sparse_masks=False, **kw)
    assert on == off and all(g.qmask for g in on)


def test_sparse_mode_needs_two_masked_groups():
    assert [g.qmask for g in _plan([{"a": 1}] * 3)] == [False]
    assert [g.qmask for g in _plan([None] * 3)] == [False]
    assert [g.qmask for g in _plan([{"a": 1}, None])] == [True, True]
    # the row-list choice comes first: one group left over is one masked search
    sizes = {1: 5000, 2: 3, 3: 4}
    groups = _plan([{"a": 1}, {"a": 2}, {"a": 3}, {"a": 1}], sizes, knob=16)
    assert [(g.rowlist, g.qmask) for g in groups] == [(False, False), (True, False), (True, False)]
    groups = _plan([{"a": 1}, {"a": 2}, None, {"a": 1}], sizes, knob=16)
    assert [(g.rowlist, g.qmask) for g in groups] == [(False, True), (True, False), (False, True)]


def test_sparse_mode_reuses_the_cuts_of_128_queries():
    from audio_rag_amd.retrieval.mi355x import qmask_calls

    filters = [{"a": i % 3} if i % 4 else None for i in range(200)]
    calls = qmask_calls(_plan(filters))
    assert [len(c[0]) for c in calls] == [128, 72]
    for idx, flt, q_mask in calls:
        for i, m in zip(idx, q_mask):
            assert (m == -1 and filters[i] is None) or flt[m] == filters[i]


def test_filter_query_masks_sparse_knob():
    from pydantic import ValidationError

    from audio_rag_amd.config import RetrievalConfig

    assert RetrievalConfig().filter_query_masks_sparse is False
    cfg = RetrievalConfig(filter_query_masks_sparse=True)
    assert cfg.filter_query_masks_sparse is True and cfg.filter_query_masks is False
    with pytest.raises(ValidationError):
        RetrievalConfig(filter_query_masks_sparse="sometimes")


def test_batcher_keeps_mixed_filters_with_the_sparse_knob():
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.retrieval.batcher import QueryBatcher
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    qb = QueryBatcher.__new__(QueryBatcher)
    qb.retriever = MI355XRetriever(RetrievalConfig(filter_query_masks_sparse=True), 256)
    assert qb._mixed_filters() is True


def _call(index=None, k=5, stride=0, n_masks=0):
    from audio_rag_amd import _armi

    return _armi.call("armi_sparse_topk_qmask", index, None, None, None, 1, k, None, stride, None,
                      n_masks, None, None, None, None, None, 0, None)


def test_sparse_qmask_entry_point_error_paths(armi_lib):
    from audio_rag_amd import _armi

    assert _armi.ABI_VERSION == 6 and _armi.ARMI_FLAG_QMASK == 16
    assert "armi_sparse_topk_qmask" in _armi.SIGNATURES
    for kw, text in (({}, "index is null"), ({"stride": -1}, "mask_stride_words"),
                     ({"n_masks": -1}, "n_masks < 0")):
        with pytest.raises(_armi.ArmiError, match=text) as e:
            _call(**kw)
        assert e.value.code == _armi.ARMI_ERR_INVALID, kw
