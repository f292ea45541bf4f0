#!/usr/bin/env python
"""Live-ingest measurements (DESIGN "Live ingest"): what RetrievalConfig.live_tail_rows buys an
add, and what the tail costs a search step. One hybrid collection of --rows x --dim synthetic
points (audio_rag_amd/synthetic.py), held twice: by a retriever with the knob off (every add
rebuilds the indexes on the next search) and by one with the knob on.

  (a) seconds from add_arrays(256 rows) to the first hybrid search result, knob off and on
  (b) the 64-query dense top-5 step and the hybrid 40 + 40 -> 20 step with the tail empty, a
      quarter full and full, beside the knob-off step over the same points (alternating)
  (c) armi_dense_tail_topk alone at those tail sizes: the fused pass against the forced general
      path (ARMI_TAIL_PASS=general)
  (d) one compaction of a full tail
  (e) the sparse stage alone, 64 queries at k = 5 and k = 40: the main SparseIndex.topk, and with a
      tail the main top-k followed by armi_sparse_tail_topk, against the forced general path
      (ARMI_TAIL_PASS=general: a native index over the tail + the list merge)

Times are host clocks around work that ends in a device synchronise. Every step is timed twice:
eagerly (search_batch as a caller runs it: Python and launch work included, which bounds these
sub-0.1-ms steps) and replayed from a HIP graph (the GPU's time for the same kernels). The result is merged into
--out (JSON, one entry per row count).

    python tools/live_ingest_bench.py --rows 100000 --out profiles/live_ingest_sparse_tail.json

--parent-json FILE stores another tree's (a) and (b) of the same row count (its own run of this tool,
in the same session on the same box) under the entry's "parent" key, for the comparison.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from audio_rag_amd import synthetic  # noqa: E402
from audio_rag_amd.config import RetrievalConfig  # noqa: E402
from audio_rag_amd.retrieval.mi355x import MI355XRetriever, QueryBatch  # noqa: E402

ADD = 256  # rows per add, (a)


def host_points(first: int, count: int, dim: int, dev):
    """(fp16 rows, per-row sparse tuples, payloads) of synthetic points [first, first + count)."""
    rows = synthetic.make_rows(first, count, dim, dev).cpu().numpy()
    ip, ix, iv = (t.cpu().numpy() for t in synthetic.make_sparse_rows(first, count, dev))
    ix = ix.astype(np.int32)
    sparse = [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(count)]
    payloads = [{"text": "", "metadata": {}} for _ in range(count)]
    return rows, sparse, payloads


def timed(fn, dev) -> float:
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def step_ms(fns: dict, dev, steps: int, warmup: int, rounds: int = 5) -> dict:
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
    """fn captured as a HIP graph (warmed up on a side stream first); returns the replay callable.
    A replay runs the step's kernels without the eager path's Python and launch work, so its time
    is the GPU's."""
    keep = []
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

    def replay():
        g.replay()
        return keep[0]

    return replay


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--tail", type=int, default=2048, help="live_tail_rows (capacity = twice)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="profiles/live_ingest_sparse_tail.json")
    ap.add_argument("--parent-json", default=None,
                    help="another tree's output of this tool: its (a) and (b) go under 'parent'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("live_ingest_bench needs the GPU")
    dev = torch.device("cuda", 0)
    n, dim = args.rows, args.dim
    cap = 2 * args.tail
    res = {"rows": n, "dim": dim, "live_tail_rows": args.tail, "tail_capacity": cap,
           "add_rows": ADD, "steps": args.steps, "device": torch.cuda.get_device_name(0)}

    def retriever(live: int) -> MI355XRetriever:
        return MI355XRetriever(RetrievalConfig(live_tail_rows=live, reproduce_sparse_drop=False,
                                               query_graphs=False), dim)

    off, on = retriever(0), retriever(args.tail)
    rows, sparse, payloads = host_points(0, n, dim, dev)
    for r in (off, on):
        r.add_arrays(rows.view(np.float16), payloads, sparse=sparse)
    del rows, sparse, payloads
    qd = synthetic.make_queries(1, 64, dim, dev, seed=9)[0]
    qi, qx, qv = synthetic.make_sparse_queries(64, dev, seed=10)
    qb = QueryBatch(dense=qd, sparse_indptr=qi, sparse_indices=qx, sparse_values=qv)

    def dense(r):
        return r.search_batch(qb, 5, search_type="dense")[0]

    def hybrid(r):
        return r.search_batch(qb, 20, search_type="hybrid")[0]

    res["first_build_s"] = {"off": timed(lambda: hybrid(off), dev), "on": timed(lambda: hybrid(on), dev)}
    extra = host_points(n, 3 * cap, dim, dev)  # the points added below
    at = 0

    def add(r, lo, hi):
        r.add_arrays(extra[0][lo:hi].view(np.float16), extra[2][lo:hi], sparse=extra[1][lo:hi])

    # (a) add 256 rows, then the first hybrid result
    a = {"off": [], "on": []}
    for _ in range(3):
        for name, r in (("off", off), ("on", on)):
            def go(r=r):
                add(r, at, at + ADD)
                hybrid(r)
            a[name].append(timed(go, dev))
        at += ADD
    res["a_add_to_first_result_s"] = {k: {"median": float(np.median(v)), "all": v} for k, v in a.items()}

    # (b), (c): tail empty / quarter / full (both retrievers hold the same points)
    on.collection().compact()
    res["b_steps_ms"], res["b_graph_steps_ms"], res["c_tail_pass_ms"] = {}, {}, {}
    res["e_sparse_stage_ms"] = {}
    for label, target in (("empty", 0), ("quarter", cap // 4), ("full", cap)):
        seg = on.collection().segments()
        have = seg.tail.n_rows if seg.tail is not None else 0
        if target > have:
            for r in (off, on):
                add(r, at, at + target - have)
            at += target - have
        hybrid(off), hybrid(on)
        seg = on.collection().segments()
        assert (seg.tail.n_rows if seg.tail is not None else 0) == target, label
        same = all(torch.equal(x, y) for x, y in zip((dense(on).ids, hybrid(on).ids),
                                                     (dense(off).ids, hybrid(off).ids)))
        fns = {"dense_off": lambda: dense(off), "dense_on": lambda: dense(on),
               "hybrid_off": lambda: hybrid(off), "hybrid_on": lambda: hybrid(on)}
        b = step_ms(fns, dev, args.steps, args.warmup)
        if target:
            os.environ["ARMI_TAIL_PASS"] = "general"
            b.update(step_ms({"dense_on_general": lambda: dense(on),
                              "hybrid_on_general": lambda: hybrid(on)}, dev, args.steps, args.warmup))
            del os.environ["ARMI_TAIL_PASS"]
        b["tail_rows"], b["ids_equal_off_on"] = target, bool(same)
        res["b_steps_ms"][label] = b
        gf = {name: graphed(fn, dev) for name, fn in fns.items()}
        if target:
            os.environ["ARMI_TAIL_PASS"] = "general"
            gf["dense_on_general"] = graphed(lambda: dense(on), dev)
            gf["hybrid_on_general"] = graphed(lambda: hybrid(on), dev)
            del os.environ["ARMI_TAIL_PASS"]
        res["b_graph_steps_ms"][label] = step_ms(gf, dev, args.steps, args.warmup)
        del gf
        if target:
            c = {}
            for k in (5, 40):
                main = seg.dense.topk(qd, k)
                ws = torch.empty(seg.tail.tail_workspace_bytes(64, k), dtype=torch.uint8, device=dev)

                def fused(k=k, main=main, ws=ws):
                    return seg.tail.tail_topk(qd, k, main, workspace=ws)

                def general(k=k, main=main, ws=ws):
                    os.environ["ARMI_TAIL_PASS"] = "general"
                    out = seg.tail.tail_topk(qd, k, main, workspace=ws)
                    del os.environ["ARMI_TAIL_PASS"]
                    return out

                c[f"k{k}"] = step_ms({"fused": fused, "general": general}, dev, args.steps, args.warmup)
                c[f"k{k}"]["graph"] = step_ms({"fused": graphed(fused, dev),
                                               "general": graphed(general, dev)}, dev, args.steps,
                                              args.warmup)
                c[f"k{k}"]["fallback_queries"] = int((fused().flags == 2).sum())
            c["tail_rows"] = target
            res["c_tail_pass_ms"][label] = c

        # (e) the sparse stage alone
        e = {"tail_rows": target}
        for k in (5, 40):
            sws = torch.empty(max(seg.sparse.workspace_bytes(64, k), 1), dtype=torch.uint8, device=dev)

            def main_only(k=k, sws=sws):
                return seg.sparse.topk(qi, qx, qv, k, workspace=sws)

            fns = {"main": main_only}
            if target:
                ts = seg.tail_sparse
                tws = torch.empty(max(ts.tail_workspace_bytes(64, k), 1), dtype=torch.uint8,
                                  device=dev)

                def fused(k=k, tws=tws, ts=ts, main_only=main_only):
                    return ts.tail_topk(qi, qx, qv, k, main_only(), workspace=tws)

                def general(k=k, ts=ts, main_only=main_only):
                    os.environ["ARMI_TAIL_PASS"] = "general"
                    out = ts.tail_topk(qi, qx, qv, k, main_only())
                    del os.environ["ARMI_TAIL_PASS"]
                    return out

                fns.update(fused=fused, general=general)
                e[f"k{k}_equal"] = bool(torch.equal(fused().ids, general().ids) and
                                        torch.equal(fused().scores, general().scores))
            e[f"k{k}"] = step_ms(fns, dev, args.steps, args.warmup)
            e[f"k{k}"]["graph"] = step_ms({name: graphed(fn, dev) for name, fn in fns.items()}, dev,
                                          args.steps, args.warmup)
        res["e_sparse_stage_ms"][label] = e

    # (d) one compaction of the full tail
    res["d_compaction_s"] = timed(lambda: on.collection().compact(), dev)
    res["rows_after"] = on.count()

    if args.parent_json:
        parent = json.loads(Path(args.parent_json).read_text()).get(str(n), {})
        res["parent"] = {key: parent[key] for key in ("a_add_to_first_result_s", "b_steps_ms",
                                                      "b_graph_steps_ms", "first_build_s")
                         if key in parent}
    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged[str(n)] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
