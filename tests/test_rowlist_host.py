"""CPU checks of the selective-filter plumbing: ChunkCollection.filter_rows against the mask
conjunction it replaces, the planner's grouping and path choice, the config knob, and the refusal
of per-query filters on a sharded retriever."""

import numpy as np
import pytest
import torch


def _collection(n: int = 600):
    from audio_rag_amd.retrieval.collection import ChunkCollection

    coll = ChunkCollection("c", 256, False, torch.device("cpu"))
    _extend(coll, 0, n)
    return coll


def _payload(i: int) -> dict:
    md = {"audio_id": i % 37, "speaker": f"s{i % 3}", "flag": i % 2 == 0,
          "tags": [f"t{i % 5}", i % 7], "score": float(i % 4) if i % 8 else 2.5}
    if i % 11 == 0:
        md["odd"] = None if i % 22 else {"a": i % 3}   # values the key index cannot classify
    if i % 13 == 0:
        del md["speaker"]
    return {"text": f"c{i}", "metadata": md}


def _extend(coll, lo: int, hi: int) -> None:
    dense = np.zeros((hi - lo, 256), dtype=np.float16)
    coll.upsert(dense, [None] * (hi - lo), [_payload(i) for i in range(lo, hi)])


def _conjunction(coll, flt: dict) -> np.ndarray:
    ok = np.ones(coll.count, dtype=bool)
    for k, v in flt.items():
        ok &= coll._key_matches(k, v, coll.count)
    return np.nonzero(ok)[0]


FILTERS = [
    {"audio_id": 5},                              # scalar
    {"speaker": "s1"},                            # string scalar, key missing on some points
    {"tags": "t3"}, {"tags": 4},                  # list-valued fields
    {"flag": True}, {"flag": 1}, {"audio_id": True},   # bool against int: classes never mix
    {"audio_id": 5.0}, {"score": 2.0}, {"score": 2.5}, {"audio_id": 5.5},   # floats
    {"audio_id": 5, "speaker": "s2"}, {"audio_id": 5, "flag": False, "tags": "t0"},   # conjunctions
    {"audio_id": 5, "speaker": "nobody"},
    {"missing": 1}, {"audio_id": 5, "missing": 1},     # a key no point has
    {"audio_id": 1000},                            # a value no point has
    {"odd": None}, {"odd": {"a": 1}}, {"audio_id": 5, "odd": None},   # the general comparison
    {"audio_id": [5]},                             # an unusual wanted value
]


@pytest.mark.parametrize("flt", FILTERS, ids=[repr(f) for f in FILTERS])
def test_filter_rows_equals_the_mask_conjunction(flt):
    coll = _collection()
    rows = coll.filter_rows(flt)
    assert rows.dtype == np.int64 and rows.ndim == 1
    np.testing.assert_array_equal(rows, _conjunction(coll, flt))
    assert (np.diff(rows) > 0).all()


def test_filter_rows_covers_every_case_kind():
    """The parametrised filters are not all empty or all full (the comparison above would pass on
    a filter_rows that returned nothing for everything only if the masks were empty too)."""
    coll = _collection()
    sizes = {repr(f): len(coll.filter_rows(f)) for f in FILTERS}
    assert sizes[repr({"audio_id": 5})] == len(range(5, 600, 37))
    assert sizes[repr({"flag": 1})] == 0 and sizes[repr({"flag": True})] == 300
    assert sizes[repr({"audio_id": 5.0})] == sizes[repr({"audio_id": 5})]
    assert sizes[repr({"score": 2.5})] == 0 and sizes[repr({"score": 2.0})] > 0
    assert sizes[repr({"missing": 1})] == 0 and sizes[repr({"odd": None})] > 0
    assert len(coll.filter_rows(None)) == len(coll.filter_rows({})) == 600


def test_filter_rows_after_an_upsert():
    coll = _collection(300)
    before = coll.filter_rows({"audio_id": 5, "flag": False})
    np.testing.assert_array_equal(before, _conjunction(coll, {"audio_id": 5, "flag": False}))
    _extend(coll, 300, 600)
    after = coll.filter_rows({"audio_id": 5, "flag": False})
    np.testing.assert_array_equal(after, _conjunction(coll, {"audio_id": 5, "flag": False}))
    assert len(after) > len(before) and after.max() >= 300
    np.testing.assert_array_equal(after[:len(before)], before)


# --------------------------------------------------------------------------------- planner

def _plan(filters, n_rows, knob, sizes):
    from audio_rag_amd.retrieval.mi355x import plan_filter_groups

    asked = []

    def count(f):
        asked.append(f)
        return sizes[f["a"]]

    return plan_filter_groups(filters, n_rows, knob, count), asked


def test_planner_knob_off_only_groups():
    filters = [{"a": 1}, None, {"a": 2}, {"a": 1}, {}, None]
    groups, asked = _plan(filters, 1000, 0, {1: 3, 2: 0})
    assert asked == []  # nothing is counted with the knob off
    assert [(g.filter, g.queries, g.rowlist) for g in groups] == [
        ({"a": 1}, [0, 3], False), (None, [1, 4, 5], False), ({"a": 2}, [2], False)]


def test_planner_path_choice():
    sizes = {1: 100, 2: 257, 3: 0, 4: 256, 5: 10}
    filters = ([{"a": 1}] * 5 + [{"a": 2}] + [None] * 2 + [{"a": 3}] * 64 + [{"a": 4}] * 2
               + [{"a": 1}] + [{"a": 5}] * 51)
    groups, asked = _plan(filters, 1024, 256, sizes)
    by = {g.filter["a"] if g.filter else None: g for g in groups}
    assert [g.filter for g in groups] == [{"a": 1}, {"a": 2}, None, {"a": 3}, {"a": 4}, {"a": 5}]
    assert sorted(f["a"] for f in asked) == [1, 2, 3, 4, 5]  # each filter counted once
    # 6 queries x 100 rows: 2 * 6 * 100 = 1200 > 1024 rows: the byte-parity bound refuses it
    assert by[1].queries == [0, 1, 2, 3, 4, 74] and by[1].matches == 100 and not by[1].rowlist
    assert not by[2].rowlist and by[2].matches == 257          # above the knob
    assert not by[None].rowlist and by[None].matches == -1      # no filter: the plain scan
    assert by[3].rowlist and len(by[3].queries) == 64           # an empty match always qualifies
    assert by[4].rowlist                                        # m = knob, 2 * 2 * 256 = 1024 <= 1024
    assert by[5].rowlist                                        # 2 * 51 * 10 = 1020 <= 1024
    groups, _ = _plan([{"a": 5}] * 51, 1019, 256, sizes)
    assert not groups[0].rowlist
    groups, _ = _plan([{"a": 5}] * 51, 1020, 256, sizes)
    assert groups[0].rowlist
    groups, _ = _plan([{"a": 1}] * 5, 1000, 256, sizes)          # 2 * 5 * 100 = 1000 <= 1000
    assert groups[0].rowlist
    groups, _ = _plan([{"a": 1}] * 5, 999, 256, sizes)
    assert not groups[0].rowlist
    groups, _ = _plan([{"a": 1}] * 5, 10**6, 99, sizes)          # m above the knob
    assert not groups[0].rowlist
    groups, _ = _plan([{"a": 3}], 0, 1, sizes)                   # empty match, empty collection
    assert groups[0].rowlist


# ---------------------------------------------------------------------------------- config

def test_filter_list_rows_knob():
    from pydantic import ValidationError

    from audio_rag_amd.config import RetrievalConfig

    assert RetrievalConfig().filter_list_rows == 0
    assert RetrievalConfig(filter_list_rows=4096).filter_list_rows == 4096
    with pytest.raises(ValidationError):
        RetrievalConfig(filter_list_rows=-1)


def test_per_query_filters_refused_on_a_sharded_retriever():
    """The collective search agrees on one filter per call: the list form raises before any device
    or collective work (a retriever made sharded by hand: no process group here)."""
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.core.exceptions import RetrievalError
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever, QueryBatch

    ret = MI355XRetriever(RetrievalConfig(filter_list_rows=256), 256)
    ret._rank, ret._world = 0, 2
    qb = QueryBatch(dense=torch.zeros((2, 256), dtype=torch.float16))
    with pytest.raises(RetrievalError, match="one filter per query"):
        ret.search_batch(qb, 5, filter_metadata=[{"audio_id": 1}, None])
    ret._world = 1
    with pytest.raises(RetrievalError, match="3 filters for 2 queries"):
        ret.search_batch(qb, 5, filter_metadata=[None, None, None])
