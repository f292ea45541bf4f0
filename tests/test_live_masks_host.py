"""CPU checks of the live-collection per-query-mask plumbing (filter_query_masks_live): what
plan_filter_groups' tail_masks lifts and what it leaves alone, the config knob, the argument
errors of armi_dense_tail_topk_qmask and armi_sparse_tail_topk_qmask (no device work) and the
two names on the library surface."""

import pytest

BROAD = [{"a": 1}, None, {"a": 2}, {"a": 1}, {}, None]
MARKED = [({"a": 1}, [0, 3], False, True), (None, [1, 4, 5], False, True),
          ({"a": 2}, [2], False, True)]


def _plan(filters, **kw):
    from audio_rag_amd.retrieval.mi355x import plan_filter_groups

    return plan_filter_groups(filters, 10000, 0, lambda f: 0, **kw)


@pytest.mark.parametrize("mode", ["dense", "legacy_dense", "hybrid"])
def test_tail_masks_lifts_the_tail_condition_of_the_dense_rule(mode):
    kw = {"mode": mode, "query_masks": True, "qmask_supported": lambda n: True, "tail_rows": 1}
    assert all(not g.qmask for g in _plan(BROAD, **kw))
    groups = _plan(BROAD, tail_masks=True, **kw)
    assert [(g.filter, g.queries, g.rowlist, g.qmask) for g in groups] == MARKED
    # the other conditions of the rule still hold
    kw["qmask_supported"] = lambda n: False
    assert all(not g.qmask for g in _plan(BROAD, tail_masks=True, **kw))
    assert [g.qmask for g in _plan([{"a": 1}] * 3, tail_masks=True, **kw)] == [False]


def test_tail_masks_lifts_the_tail_condition_of_the_sparse_rule():
    kw = {"mode": "sparse", "sparse_masks": True, "tail_rows": 1}
    assert all(not g.qmask for g in _plan(BROAD, **kw))
    groups = _plan(BROAD, tail_masks=True, **kw)
    assert [(g.filter, g.queries, g.rowlist, g.qmask) for g in groups] == MARKED


@pytest.mark.parametrize("mode", ["dense", "legacy_dense", "hybrid", "sparse"])
@pytest.mark.parametrize("tail_rows", [0, 1])
def test_tail_masks_alone_marks_nothing(mode, tail_rows):
    # both knobs off: the index's answer is not enough
    groups = _plan(BROAD, mode=mode, tail_rows=tail_rows, tail_masks=True,
                   qmask_supported=lambda n: True)
    assert all(not g.qmask and not g.rowlist for g in groups)
    # a single group is one masked search whatever the knobs say
    one = _plan([{"a": 1}] * 4, mode=mode, tail_rows=tail_rows, tail_masks=True, query_masks=True,
                sparse_masks=True, qmask_supported=lambda n: True)
    assert [(g.queries, g.qmask) for g in one] == [([0, 1, 2, 3], False)]
    # the dense index refuses the shape: dense modes stay as they were
    if mode != "sparse":
        no = _plan(BROAD, mode=mode, tail_rows=tail_rows, tail_masks=True, query_masks=True,
                   qmask_supported=lambda n: False)
        assert all(not g.qmask for g in no)


def test_tail_masks_defaults_to_false():
    import inspect

    from audio_rag_amd.retrieval.mi355x import plan_filter_groups

    assert inspect.signature(plan_filter_groups).parameters["tail_masks"].default is False
    kw = {"query_masks": True, "qmask_supported": lambda n: True, "sparse_masks": True}
    for mode in ("dense", "legacy_dense", "hybrid", "sparse"):
        assert all(not g.qmask for g in _plan(BROAD, mode=mode, tail_rows=1, **kw))
        assert all(g.qmask for g in _plan(BROAD, mode=mode, tail_rows=0, **kw))


def test_tail_masks_leaves_a_collection_without_tail_rows_alone():
    for mode in ("dense", "hybrid", "sparse"):
        kw = {"mode": mode, "query_masks": True, "qmask_supported": lambda n: True,
              "sparse_masks": True}
        assert _plan(BROAD, tail_masks=True, **kw) == _plan(BROAD, tail_masks=False, **kw)


def test_filter_query_masks_live_knob():
    from pydantic import ValidationError

    from audio_rag_amd.config import RetrievalConfig

    assert RetrievalConfig().filter_query_masks_live is False
    cfg = RetrievalConfig(filter_query_masks_live=True)
    assert cfg.filter_query_masks_live is True
    assert cfg.filter_query_masks is False and cfg.filter_query_masks_sparse is False
    with pytest.raises(ValidationError):
        RetrievalConfig(filter_query_masks_live="sometimes")


def _dense(index=None, k=5, stride=0, n_masks=0):
    from audio_rag_amd import _armi

    return _armi.call("armi_dense_tail_topk_qmask", index, None, 1, k, None, stride, None, n_masks,
                      None, None, None, None, None, None, None, None, None, None, 0, None)


def _sparse(tail_rows=0, k=5, stride=0, n_masks=0):
    from audio_rag_amd import _armi

    return _armi.call("armi_sparse_tail_topk_qmask", None, None, None, tail_rows, 0, None, None,
                      None, 1, k, None, stride, None, n_masks, None, None, None, None, None, None,
                      None, None, None, 0, None)


@pytest.mark.parametrize("fn,kw,text", [
    (_dense, {}, "index is null"),
    (_dense, {"n_masks": -1}, "n_masks < 0"),
    (_dense, {"stride": -1}, "mask_stride_words"),
    (_dense, {"k": 0}, r"k must be in \[1, 240\]"),
    (_dense, {"k": 241}, r"k must be in \[1, 240\]"),
    (_sparse, {"tail_rows": 100, "stride": 2}, "null pointer"),       # a null CSR
    (_sparse, {}, "null pointer"),                                    # a null query CSR
    (_sparse, {"n_masks": -1}, "n_masks < 0"),
    (_sparse, {"tail_rows": 129, "stride": 2}, "mask_stride_words"),  # 129 rows need 3 words
    (_sparse, {"stride": -1}, "mask_stride_words"),
    (_sparse, {"k": 0}, r"k must be in \[1, 240\]"),
    (_sparse, {"k": 241}, r"k must be in \[1, 240\]"),
], ids=["dense-null-index", "dense-n_masks", "dense-stride", "dense-k0", "dense-k241",
        "sparse-null-csr", "sparse-null-queries", "sparse-n_masks", "sparse-short-stride",
        "sparse-stride", "sparse-k0", "sparse-k241"])
def test_tail_qmask_entry_point_error_paths(armi_lib, fn, kw, text):
    from audio_rag_amd import _armi

    with pytest.raises(_armi.ArmiError, match=text) as e:
        fn(**kw)
    assert e.value.code == _armi.ARMI_ERR_INVALID


def test_the_two_names_are_on_every_surface(armi_lib):
    from audio_rag_amd import _armi

    assert _armi.ABI_VERSION == 6 and armi_lib.armi_abi_version() == 6
    header = _armi.HEADER.read_text()
    for name in ("armi_dense_tail_topk_qmask", "armi_sparse_tail_topk_qmask"):
        assert name in _armi.SIGNATURES
        assert f"int {name}(" in header
        assert getattr(armi_lib, name) is not None
