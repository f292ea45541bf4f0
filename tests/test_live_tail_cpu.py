"""CPU checks of the live-ingest plumbing: the per-segment row masks and the config knob."""

import numpy as np
import pytest


def _bit(words: np.ndarray, r: int) -> bool:
    return bool((int(words[r >> 6]) >> (r & 63)) & 1)


@pytest.mark.parametrize("n,main_rows", [(300, 100), (1000, 77), (130, 129), (64, 64), (200, 0),
                                         (5, 5), (4097, 4033)])
def test_segment_masks_split_at_any_row(n, main_rows):
    from audio_rag_amd.retrieval.collection import mask_words, split_mask_words

    ok = np.random.default_rng(n + main_rows).random(n) < 0.4
    main, tail = split_mask_words(ok, main_rows)
    assert main.dtype == tail.dtype == np.uint64
    assert len(main) == max((main_rows + 63) // 64, 1)
    assert len(tail) == max((n - main_rows + 63) // 64, 1)
    assert [_bit(main, r) for r in range(main_rows)] == ok[:main_rows].tolist()
    # the tail's bit 0 is the tail's first row, wherever that row falls in the whole mask's words
    assert [_bit(tail, r) for r in range(n - main_rows)] == ok[main_rows:].tolist()
    # nothing set past either segment's end
    assert sum(bin(int(w)).count("1") for w in main) == int(ok[:main_rows].sum())
    assert sum(bin(int(w)).count("1") for w in tail) == int(ok[main_rows:].sum())
    np.testing.assert_array_equal(mask_words(ok)[:len(main) - 1], main[:len(main) - 1])


def test_live_tail_rows_knob():
    from pydantic import ValidationError

    from audio_rag_amd.config import RetrievalConfig

    assert RetrievalConfig().live_tail_rows == 0
    assert RetrievalConfig(live_tail_rows=256).live_tail_rows == 256
    with pytest.raises(ValidationError):
        RetrievalConfig(live_tail_rows=-1)


def test_collection_defaults_to_rebuild():
    """The knob off, sharded collections and collections without host staging never keep a tail."""
    import torch

    from audio_rag_amd.retrieval.collection import ChunkCollection

    dev = torch.device("cpu")
    assert not ChunkCollection("c", 256, False, dev)._live
    assert ChunkCollection("c", 256, False, dev, live_tail_rows=64)._live
    assert not ChunkCollection("c", 256, False, dev, live_tail_rows=64, shard=(1, 2))._live
    assert not ChunkCollection("c", 256, False, dev, live_tail_rows=64, _frozen=True)._live
