"""CPU checks of the per-query-mask plumbing (filter_query_masks): which groups the planner marks
`qmask` under each of its conditions, how their queries are cut into calls and their masks
stacked, the config knob, and the C entry point's argument errors (no device work)."""

import pytest


def _plan(filters, sizes=None, knob=0, n_rows=10000, **kw):
    from audio_rag_amd.retrieval.mi355x import plan_filter_groups

    kw.setdefault("query_masks", True)
    kw.setdefault("qmask_supported", lambda n: True)
    return plan_filter_groups(filters, n_rows, knob, lambda f: (sizes or {})[f["a"]], **kw)


BROAD = [{"a": 1}, None, {"a": 2}, {"a": 1}, {}, None]


def test_planner_marks_every_masked_group_the_unfiltered_one_included():
    groups = _plan(BROAD)
    assert [(g.filter, g.queries, g.rowlist, g.qmask) for g in groups] == [
        ({"a": 1}, [0, 3], False, True), (None, [1, 4, 5], False, True),
        ({"a": 2}, [2], False, True)]


def test_planner_default_is_off():
    from audio_rag_amd.retrieval.mi355x import FilterGroup, plan_filter_groups

    assert FilterGroup(None, []).qmask is False
    groups = plan_filter_groups(BROAD, 10000, 0, lambda f: 0)
    assert all(not g.qmask and not g.rowlist for g in groups)


@pytest.mark.parametrize("kw", [
    {"query_masks": False},                     # the knob
    {"mode": "sparse"},                         # the sparse kernels have no such form
    {"tail_rows": 1},                           # a live tail
    {"qmask_supported": lambda n: False},       # k > 64, no int8 image
    {"qmask_supported": None},
], ids=["knob", "sparse", "tail", "unsupported", "no-index-answer"])
def test_planner_conditions(kw):
    assert all(not g.qmask for g in _plan(BROAD, **kw))
    assert all(g.qmask for g in _plan(BROAD))


@pytest.mark.parametrize("mode", ["dense", "legacy_dense", "hybrid"])
def test_planner_modes(mode):
    assert all(g.qmask for g in _plan(BROAD, mode=mode))


def test_planner_needs_two_masked_groups():
    assert [g.qmask for g in _plan([{"a": 1}] * 3)] == [False]
    assert [g.qmask for g in _plan([None] * 3)] == [False]
    assert [g.qmask for g in _plan([{"a": 1}, None])] == [True, True]
    # the row-list choice comes first: one group left over is one masked search
    sizes = {1: 5000, 2: 3, 3: 4}
    groups = _plan([{"a": 1}, {"a": 2}, {"a": 3}, {"a": 1}], sizes, knob=16)
    assert [(g.rowlist, g.qmask) for g in groups] == [(False, False), (True, False), (True, False)]
    groups = _plan([{"a": 1}, {"a": 2}, None, {"a": 1}], sizes, knob=16)
    assert [(g.rowlist, g.qmask) for g in groups] == [(False, True), (True, False), (False, True)]


def test_planner_asks_support_for_the_calls_size():
    asked = []

    def supported(n):
        asked.append(n)
        return True

    _plan([{"a": 1}] * 40 + [None] * 30, qmask_supported=supported)
    _plan([{"a": 1}] * 100 + [None] * 100, qmask_supported=supported)
    assert asked == [70, 128]


def test_qmask_calls_stacking_and_q_mask():
    from audio_rag_amd.retrieval.mi355x import qmask_calls

    filters = [{"a": 2}, None, {"a": 1}, {"a": 2}, {}, {"a": 3}, {"a": 1}]
    sizes = {1: 5000, 2: 5000, 3: 2}
    groups = _plan(filters, sizes, knob=16)     # {"a": 3} goes to its row list
    calls = qmask_calls(groups)
    assert len(calls) == 1
    idx, flt, q_mask = calls[0]
    assert idx == [0, 3, 1, 4, 2, 6]            # the groups' order, a group's queries together
    assert flt == [{"a": 2}, {"a": 1}]          # distinct filters, first appearance; no None row
    assert q_mask == [0, 0, -1, -1, 1, 1]       # repeated filters share a row
    assert qmask_calls(_plan(filters, sizes, knob=16, query_masks=False)) == []


def test_qmask_calls_chunks_of_128():
    from audio_rag_amd.retrieval.mi355x import QMASK_MAX_QUERIES, qmask_calls

    assert QMASK_MAX_QUERIES == 128
    filters = [{"a": i % 3} if i % 4 else None for i in range(300)]
    calls = qmask_calls(_plan(filters))
    assert [len(c[0]) for c in calls] == [128, 128, 44]
    assert sorted(i for c in calls for i in c[0]) == list(range(300))
    for idx, flt, q_mask in calls:
        assert len(q_mask) == len(idx) and len(flt) <= 3
        for i, m in zip(idx, q_mask):           # every query names its own filter's row
            assert (m == -1 and filters[i] is None) or flt[m] == filters[i]
        assert sorted(set(q_mask) - {-1}) == list(range(len(flt)))   # rows are per call


def test_filter_query_masks_knob():
    from pydantic import ValidationError

    from audio_rag_amd.config import RetrievalConfig

    assert RetrievalConfig().filter_query_masks is False
    assert RetrievalConfig(filter_query_masks=True).filter_query_masks is True
    with pytest.raises(ValidationError):
        RetrievalConfig(filter_query_masks="sometimes")


def test_qmask_entry_point_error_path(armi_lib):
    from audio_rag_amd import _armi

    assert _armi.ABI_VERSION == 6 and _armi.ARMI_FLAG_QMASK == 16
    with pytest.raises(_armi.ArmiError, match="index is null") as e:
        _armi.call("armi_dense_topk_qmask", None, None, 1, 5, None, 0, None, 0, None, None, None,
                   None, None, None, 0, None)
    assert e.value.code == _armi.ARMI_ERR_INVALID
    assert _armi.query("armi_dense_qmask_supported", None, 1, 5) == 0
    assert _armi.query("armi_dense_qmask_workspace_bytes", None, 1, 5, 1) == 0


def test_batcher_keeps_mixed_filters_with_the_knob():
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.retrieval.batcher import QueryBatcher
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    for cfg, want in ((RetrievalConfig(), False), (RetrievalConfig(filter_query_masks=True), True),
                      (RetrievalConfig(filter_list_rows=8), True)):
        qb = QueryBatcher.__new__(QueryBatcher)
        qb.retriever = MI355XRetriever(cfg, 256)
        assert qb._mixed_filters() is want
