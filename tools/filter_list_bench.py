#!/usr/bin/env python
"""Selective-filter measurements (DESIGN "Selective filters"): what RetrievalConfig.filter_list_rows
buys a filtered search. One hybrid collection of --rows x --dim synthetic points
(audio_rag_amd/synthetic.py) with block-valued metadata (a "recording" = m consecutive chunks),
served by two retrievers over the same device indexes: knob off (every filter a masked scan of the
whole index, one search per filter: what the code did before the knob) and knob on.
64-query batches, dense top-5 and hybrid 40 + 40 -> 20.

  (a) 64 distinct filters matching m rows each (m = 64, 1k, 16k; "16k" is rows / 64 = 15,625 at
      1M rows, where 64 x 16,000 rows do not fit, and is skipped below 512k rows), off against on
  (b) one filter shared by all 64 queries at m = 1k, 8k, 64k, rows / 128: the masked scan against
      the row-list path FORCED (whatever the planner's byte-parity rule says), to locate the real
      crossover beside the rule's (2 * 64 * m <= rows, i.e. m <= rows / 128)
  (c) single-query search() p50 with a 1k-row filter, off against on
  (d) the unfiltered 64-query step on both retrievers (the same kernels)

Times are host clocks around work that ends in a device synchronise. Steps are timed eagerly
(search_batch as a caller runs it: the planner, Python and launch work included) and, where the
path is device work only, replayed from a HIP graph (the GPU's time for the same kernels): the
row-list launches of (a) and (b), the masked scans of (b) and (d). The result is merged into --out
(JSON, one entry per row count).

    python tools/filter_list_bench.py --rows 100000 --out profiles/filter_list.json
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from audio_rag_amd import synthetic  # noqa: E402
from audio_rag_amd.config import RetrievalConfig  # noqa: E402
from audio_rag_amd.core import EmbeddingResult, SparseVector  # noqa: E402
from audio_rag_amd.retrieval.collection import ChunkCollection  # noqa: E402
from audio_rag_amd.retrieval.device import DenseIndex, SparseIndex  # noqa: E402
from audio_rag_amd.retrieval.mi355x import FilterGroup, MI355XRetriever, QueryBatch  # noqa: E402

B = 64
A_SIZES = {"64": 64, "1k": 1000, "16k": 16000}  # (a): rows per recording ("16k": see a_sizes)


def timed(fn, dev) -> float:
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def step_ms(fns: dict, dev, steps: int, warmup: int, rounds: int = 3) -> dict:
    """Median over `rounds` of the mean step time (ms) of each named step, the steps alternating
    round by round (other work shares the host)."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    acc = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            acc[name].append(timed(lambda: [fn() for _ in range(steps)], dev) / steps * 1e3)
    return {name: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}
            for name, v in acc.items()}


def graphed(fn, dev):
    """fn captured as a HIP graph (warmed up on a side stream first); returns the replay callable,
    or None when the capture is refused."""
    keep = []
    try:
        with torch.inference_mode():
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(2):
                    fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep.append(fn())
    except RuntimeError as e:
        print(f"capture refused: {e}", file=sys.stderr)
        return None

    def replay():
        g.replay()
        return keep[0]

    return replay


def a_sizes(n: int) -> dict:
    """(a)'s recording sizes for n rows: 64 recordings of each size have to fit, so the largest is
    min(16,000, n / 64), and is left out when that is under 8,000 rows."""
    sizes = dict(A_SIZES)
    sizes["16k"] = min(sizes["16k"], n // B)
    return sizes


def payloads(n: int, shared: dict) -> list[dict]:
    """Metadata of point i: a<m> = i // m for the first 64 m points (64 recordings of m chunks),
    b<m> = True for the first m points (one recording shared by a whole batch)."""
    out = []
    sizes = a_sizes(n)
    for i in range(n):
        md = {f"a{name}": i // m for name, m in sizes.items() if i < B * m}
        md.update({f"b{name}": True for name, m in shared.items() if i < m})
        out.append({"text": "", "metadata": md})
    return out


def rowlist_queries(t) -> int:
    """Queries of a result answered by the row-list path (ARMI_FLAG_ROWLIST)."""
    return 0 if t.flags is None else int(((t.flags & 8) != 0).sum())


def same(x, y, mode: str) -> bool:
    sc = (lambda t: t.rank) if mode == "hybrid" else (lambda t: t.scores)
    return bool(torch.equal(x.ids, y.ids) and torch.equal(x.count, y.count)
                and torch.equal(sc(x), sc(y)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/filter_list.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filter_list_bench needs the GPU")
    dev = torch.device("cuda", 0)
    n, dim = args.rows, args.dim
    shared = {"1k": 1000, "8k": 8000, "64k": 64000, "n128": n // 128}
    res = {"rows": n, "dim": dim, "batch": B, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), "rule_crossover_rows": n // (2 * B)}

    dense = DenseIndex(synthetic.make_rows(0, n, dim, dev))
    sparse = SparseIndex(*synthetic.make_sparse_rows(0, n, dev), vocab=synthetic.VOCAB)
    coll = ChunkCollection.from_indexes("audio_rag", dense, payloads(n, shared), sparse)

    def retriever(knob: int) -> MI355XRetriever:
        r = MI355XRetriever(RetrievalConfig(filter_list_rows=knob, reproduce_sparse_drop=False,
                                            query_graphs=False), dim)
        r.attach_collection(coll)
        return r

    off, on = retriever(0), retriever(n)  # knob = rows: the byte-parity rule alone decides
    qd = synthetic.make_queries(1, B, dim, dev, seed=9)[0]
    qi, qx, qv = synthetic.make_sparse_queries(B, dev, seed=10)
    qb = QueryBatch(dense=qd, sparse_indptr=qi, sparse_indices=qx, sparse_values=qv)
    modes = {"dense": 5, "hybrid": 20}
    seg = coll.segments()

    def search(r, mode, flt):
        return r.search_batch(qb, modes[mode], filter_metadata=flt, search_type=mode)[0]

    def forced(mode, groups):
        """The row-list launches alone for the whole batch in the groups' order (lists encoded
        once: device work only)."""
        main, tail = on._encode_rowlists(coll, groups)
        return lambda: on._search_rowlists(seg, qb, modes[mode], mode, main, tail)

    # (a) 64 distinct filters
    res["a_distinct_filters_ms"] = {}
    for name, m in a_sizes(n).items():
        if name == "16k" and m < 8000:
            res["a_distinct_filters_ms"][name] = {"skipped": f"64 x 16000 rows exceed {n}"}
            continue
        flt = [{f"a{name}": q} for q in range(B)]
        entry = {"match_rows": m}
        for mode in modes:
            x, y = search(off, mode, flt), search(on, mode, flt)
            entry[mode] = step_ms({"off": lambda: search(off, mode, flt),
                                   "on": lambda: search(on, mode, flt)}, dev, args.steps, args.warmup)
            entry[mode]["equal"] = same(x, y, mode)
            entry[mode]["rowlist_queries"] = rowlist_queries(y)
            groups = [FilterGroup(f, [q], m, True) for q, f in enumerate(flt)]
            g = graphed(forced(mode, groups), dev)
            if g is not None:
                entry[mode]["on_graph"] = step_ms({"on": g}, dev, args.steps, args.warmup)["on"]
        res["a_distinct_filters_ms"][name] = entry

    # (b) one filter shared by the batch: masked scan against the forced row-list path
    res["b_shared_filter_ms"] = {}
    for name, m in shared.items():
        if m > n or m == 0:
            continue
        flt = {f"b{name}": True}
        entry = {"match_rows": m, "rule_takes_list": 2 * B * m <= n}
        group = [FilterGroup(flt, list(range(B)), m, True)]
        masks = coll.segment_masks(flt)
        for mode in modes:
            scan = lambda mode=mode: off._search_device(coll, qb, modes[mode], mode, masks)
            lst = forced(mode, group)
            entry[mode] = step_ms({"scan": scan, "list": lst}, dev, args.steps, args.warmup)
            entry[mode]["equal"] = same(scan(), lst(), mode)
            gs, gl = graphed(scan, dev), graphed(lst, dev)
            if gs is not None and gl is not None:
                entry[mode]["graph"] = step_ms({"scan": gs, "list": gl}, dev, args.steps, args.warmup)
            entry[mode]["planner_rowlist_queries"] = rowlist_queries(search(on, mode, flt))
        res["b_shared_filter_ms"][name] = entry

    # (c) single-query search() with a 1k-row filter
    qh, ih, xh, vh = qd.cpu().float().numpy(), qi.cpu().numpy(), qx.cpu().numpy(), qv.cpu().numpy()
    embs = [EmbeddingResult(dense=qh[q].tolist(), sparse=SparseVector(
        xh[ih[q]:ih[q + 1]].tolist(), vh[ih[q]:ih[q + 1]].tolist())) for q in range(B)]
    res["c_single_query_ms"] = {}
    for mode in modes:
        lat = {"off": [], "on": []}
        for rnd in range(3):
            for q, emb in enumerate(embs):
                for name, r in (("off", off), ("on", on)):
                    t = timed(lambda: r.search(emb, modes[mode], filter_metadata={"a1k": q},
                                               search_type=mode), dev)
                    if rnd:
                        lat[name].append(t * 1e3)
        res["c_single_query_ms"][mode] = {k: {"p50": float(np.percentile(v, 50)),
                                              "p99": float(np.percentile(v, 99))}
                                          for k, v in lat.items()}

    # (d) the unfiltered step
    res["d_unfiltered_ms"] = {}
    for mode in modes:
        fns = {"off": lambda: search(off, mode, None), "on": lambda: search(on, mode, None)}
        entry = step_ms(fns, dev, 10 * args.steps, args.warmup)
        gf = {k: graphed(f, dev) for k, f in fns.items()}
        if all(g is not None for g in gf.values()):
            entry["graph"] = step_ms(gf, dev, 10 * args.steps, args.warmup)
        res["d_unfiltered_ms"][mode] = entry

    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged[str(n)] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
