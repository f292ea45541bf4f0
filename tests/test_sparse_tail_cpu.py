"""CPU checks of the append-only sparse tail: the CSR-append helper on host tensors and the sizing
entry points of armi_sparse_tail_topk (no kernel runs here)."""

import numpy as np
import pytest
import torch


def _block(rng, lens):
    """A CSR of its own for rows of the given posting counts (indptr from 0)."""
    ip = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    ix = np.concatenate([np.sort(rng.choice(5000, size=n, replace=False)) for n in lens] +
                        [np.zeros(0, np.int64)]).astype(np.int32)
    iv = rng.uniform(0.01, 0.4, size=int(ip[-1])).astype(np.float32)
    return ip, ix, iv


def _host_concat(blocks):
    ip, end = [np.zeros(1, dtype=np.int64)], 0
    for b in blocks:
        ip.append(b[0][1:] + end)
        end += int(b[0][-1])
    return (np.concatenate(ip), np.concatenate([b[1] for b in blocks]),
            np.concatenate([b[2] for b in blocks]))


@pytest.mark.parametrize("lens", [
    [[3, 1, 7], [2, 2], [5]],            # three blocks
    [[0, 4, 0], [0], [0, 0, 6, 0]],      # rows without postings, first / last / alone
    [[2, 3], [], [4]],                   # an empty block in the middle
    [[], [1, 2], []],                    # the first append and the last are empty blocks
    [[0, 0], [0]],                       # no posting at all
])
def test_csr_append_equals_the_host_concatenation(lens):
    from audio_rag_amd.retrieval.device import csr_append

    rng = np.random.default_rng(1)
    blocks = [_block(rng, b) for b in lens]
    csr = (None, None, None)
    for i, b in enumerate(blocks):
        new = tuple(torch.from_numpy(a) for a in b)
        old = csr
        before = tuple(None if t is None else t.clone() for t in old)
        csr = csr_append(*old, *new)
        # pure: neither the old arrays nor the block are written
        for t, kept in zip(old, before):
            assert t is None or torch.equal(t, kept)
        for a, t in zip(b, new):
            assert np.array_equal(a, t.numpy())
        want = _host_concat(blocks[:i + 1])
        assert csr[0].dtype == torch.int64 and csr[1].dtype == torch.int32
        assert csr[2].dtype == torch.float32
        for got, w in zip(csr, want):
            np.testing.assert_array_equal(got.numpy(), w)
    assert int(csr[0][0]) == 0 and int(csr[0][-1]) == csr[1].numel() == csr[2].numel()
    assert csr[0].numel() == sum(len(b) for b in lens) + 1


def test_csr_append_refuses_other_dtypes():
    from audio_rag_amd.retrieval.device import csr_append

    ip = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError):
        csr_append(None, None, None, ip.to(torch.int32), torch.zeros(0, dtype=torch.int32),
                   torch.zeros(0, dtype=torch.float32))
    with pytest.raises(ValueError):
        csr_append(None, None, None, ip, torch.zeros(1, dtype=torch.int32),
                   torch.zeros(0, dtype=torch.float32))


def test_tail_chunk_rows_and_workspace_sizes(armi_lib):
    from audio_rag_amd import _armi

    c = _armi.query("armi_sparse_tail_chunk_rows")
    assert c > 0
    ws = lambda rows, nq, k: int(_armi.query("armi_sparse_tail_workspace_bytes", rows, nq, k))
    # nothing to do: no bytes (the convention of armi_sparse_rowlist_workspace_bytes)
    assert ws(0, 64, 40) == ws(4096, 0, 40) == ws(4096, 64, 0) == ws(-1, 64, 40) == 0
    rows = [1, c - 1, c, c + 1, 2 * c, 2 * c + 70, 4096, 100_000]
    for nq in (1, 64, 70):
        for k in (1, 5, 40, 240):
            sizes = [ws(r, nq, k) for r in rows]
            assert all(a <= b for a, b in zip(sizes, sizes[1:]))
            # a tail of one chunk is finished by its scan workgroup: no workspace
            assert sizes[0] == sizes[1] == sizes[2] == 0 < sizes[3]
    for r in (c, 2 * c + 70, 4096):
        for k in (5, 240):
            sizes = [ws(r, nq, k) for nq in (1, 2, 64, 70, 65535)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:]))
        for nq in (1, 64):
            sizes = [ws(r, nq, k) for k in (1, 5, 40, 128, 240)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    # several chunks: a count and a k-entry list (key, ordinal) per query and chunk
    assert ws(2 * c + 70, 64, 40) >= 64 * 3 * (4 + 40 * 16)
