"""CPU checks of the per-query-mask pointer-table entry points and the query-masks stream server:
the five names are on every surface, the ABI version did not move, and every new call refuses a
null index / server with ARMI_ERR_INVALID and a message before any device work (no GPU here)."""

import ctypes
import inspect

import pytest

NAMES = ("armi_dense_topk_qmask_ptrs", "armi_sparse_topk_qmask_ptrs", "armi_stream_create_ex",
         "armi_stream_stats_ex", "armi_stream_loadgen_ex")


def test_the_five_names_are_on_every_surface(armi_lib):
    from audio_rag_amd import _armi

    header = _armi.HEADER.read_text()
    for name in NAMES:
        assert name in _armi.SIGNATURES
        assert f"int {name}(" in header
        assert getattr(armi_lib, name) is not None
    assert "#define ARMI_STREAM_QUERY_MASKS 1u" in header
    assert _armi.ARMI_STREAM_QUERY_MASKS == 1
    assert _armi.ABI_VERSION == 6 and armi_lib.armi_abi_version() == 6
    assert "#define ARMI_ABI_VERSION 6" in header


def test_stream_server_has_the_keyword():
    from audio_rag_amd.retrieval.batcher import StreamServer

    p = inspect.signature(StreamServer.__init__).parameters
    assert "query_masks" in p and p["query_masks"].default is False
    assert "filters" in inspect.signature(StreamServer.loadgen).parameters
    assert callable(StreamServer.stats_ex)


def _dense_ptrs():
    from audio_rag_amd import _armi

    _armi.call("armi_dense_topk_qmask_ptrs", None, None, 1, 5, None, None, 0, None, None, None,
               None, None, None, 0, None)


def _sparse_ptrs():
    from audio_rag_amd import _armi

    _armi.call("armi_sparse_topk_qmask_ptrs", None, None, None, None, 1, 5, None, None, 0, None,
               None, None, None, None, 0, None)


def _create_ex():
    from audio_rag_amd import _armi

    h = ctypes.c_void_p()
    _armi.call("armi_stream_create_ex", None, None, 5, 2, 16, 1000.0,
               _armi.ARMI_STREAM_QUERY_MASKS, ctypes.byref(h))


def _stats_ex():
    from audio_rag_amd import _armi

    b, q, m = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _armi.call("armi_stream_stats_ex", None, ctypes.byref(b), ctypes.byref(q), ctypes.byref(m))


def _loadgen_ex():
    from audio_rag_amd import _armi

    el, done = ctypes.c_double(), ctypes.c_int64()
    _armi.call("armi_stream_loadgen_ex", None, None, None, None, None, 1, 1, 100.0, 0, None, 0,
               None, ctypes.byref(el), ctypes.byref(done), None, None)


@pytest.mark.parametrize("fn,text", [
    (_dense_ptrs, "armi_dense_topk_qmask_ptrs: index is null"),
    (_sparse_ptrs, "armi_sparse_topk_qmask_ptrs: index is null"),
    (_create_ex, "null pointer"),
    (_stats_ex, "armi_stream_stats_ex: null pointer"),
    (_loadgen_ex, "armi_stream_loadgen: null pointer"),
], ids=["dense", "sparse", "create_ex", "stats_ex", "loadgen_ex"])
def test_a_null_index_or_server_is_invalid(armi_lib, fn, text):
    from audio_rag_amd import _armi

    with pytest.raises(_armi.ArmiError, match=text) as e:
        fn()
    assert e.value.code == _armi.ARMI_ERR_INVALID
    assert armi_lib.armi_last_error()          # the message is kept for the caller


@pytest.mark.parametrize("fn,kw", [
    ("dense", {"n_masks": -1}), ("dense", {"k": 0}), ("dense", {"k": 241}),
    ("sparse", {"n_masks": -1}), ("sparse", {"k": 0}),
], ids=["dense-n_masks", "dense-k0", "dense-k241", "sparse-n_masks", "sparse-k0"])
def test_argument_checks_that_need_no_index(armi_lib, fn, kw):
    """What the entry points can refuse without looking at an index comes before, or with, the
    null-index answer: always ARMI_ERR_INVALID."""
    from audio_rag_amd import _armi

    k, n_masks = kw.get("k", 5), kw.get("n_masks", 0)
    with pytest.raises(_armi.ArmiError) as e:
        if fn == "dense":
            _armi.call("armi_dense_topk_qmask_ptrs", None, None, 1, k, None, None, n_masks, None,
                       None, None, None, None, None, 0, None)
        else:
            _armi.call("armi_sparse_topk_qmask_ptrs", None, None, None, None, 1, k, None, None,
                       n_masks, None, None, None, None, None, 0, None)
    assert e.value.code == _armi.ARMI_ERR_INVALID
