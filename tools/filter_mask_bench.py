#!/usr/bin/env python
"""Per-query-mask measurements (DESIGN "Broad filters in one scan"): what
RetrievalConfig.filter_query_masks buys a batch whose queries carry different broad filters. One
hybrid collection of --rows x --dim synthetic points (audio_rag_amd/synthetic.py) with eight
metadata keys k0..k7 of eight values each (every filter {k_j: v} matches rows / 8), served by two
retrievers over the same device indexes: knob off (one masked search per filter: what the code did
before the knob) and knob on. 64-query batches, dense top-5 and hybrid 40 + 40 -> 20.

  (a) 64 distinct filters of rows / 8 rows each (no group passes filter_list_rows' byte parity)
  (b) 32 unfiltered queries and 32 under one broad filter
  (c) one filter shared by all 64 queries (the same path on and off)
  (d) the unfiltered step (the same path on and off)

Times are host clocks around work that ends in a device synchronise: search_batch as a caller runs
it (planner, Python and launch work included), the two retrievers alternating round by round. The
dense legs of (a) and (b) are also replayed from HIP graphs (the GPU's time for the same kernels:
64 / 2 masked DenseIndex.topk calls against one DenseIndex.topk_masks). For (a), the launch time of
the qmask scan kernel and of the mask-image kernel (armi_kernel_timing_read) beside the plain masked
int8 scan's, measured the same way. The result is merged into --out (JSON, one entry per row
count).

--sparse measures RetrievalConfig.filter_query_masks_sparse instead (DESIGN "Sparse search: one
row mask per query"): the same collection, cases and protocol with mode sparse top-20 and hybrid
40 + 40 -> 20; "off" is filter_query_masks alone (one masked sparse search per filter: what the
code did before the sparse knob), "on" both knobs. Kernel times (ARMI_TIMING_SPARSE_SCAN, the MFMA
filter scan of a 64-query pass at k = 20): sparse_filter_scan_kernel under one shared mask, its
per-query sibling under (a)'s 64 masks, and the unmasked scan.

--live measures RetrievalConfig.filter_query_masks_live (DESIGN "Live collections: one row mask
per query in the tail passes"): a live collection (live_tail_rows) of --rows points built once,
then a tail of 1,024 rows and one of 4,096, cases (a) and (b), modes dense top-5, sparse top-20 and
hybrid 40 + 40 -> 20; "off" is filter_query_masks + filter_query_masks_sparse (with tail rows: one
masked search and one tail pass per filter), "on" adds filter_query_masks_live. Median [min-max]
over five alternating rounds. --package-root DIR imports audio_rag_amd from another tree (the
parent commit's, with its own built library), which has no such knob and gives the "off" column
only; --parent-json FILE then stores that run under "parent" beside this tree's, with the ratio
of the parent's step to this tree's knob-on step, this tree's knob-off step against the parent's
(the same kernels: the resolution of the comparison) and whether the two trees' answers are equal
(sha256 of ids, counts and scores).

    python tools/filter_mask_bench.py --rows 100000 --out profiles/filter_masks.json
    python tools/filter_mask_bench.py --sparse --rows 100000 --out profiles/sparse_query_masks.json
    python tools/filter_mask_bench.py --live --rows 1000000 --package-root ../parent --out p.json
    python tools/filter_mask_bench.py --live --rows 1000000 --parent-json p.json \
        --out profiles/live_query_masks.json
"""

from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
# (--package-root is read before the package is imported)
_root = [a.split("=", 1)[1] if "=" in a else sys.argv[i + 1] for i, a in enumerate(sys.argv)
         if a == "--package-root" or a.startswith("--package-root=")]
sys.path.insert(0, str(Path(_root[0]).resolve() if _root else Path(__file__).resolve().parent.parent))

from audio_rag_amd import _armi, synthetic  # noqa: E402
from audio_rag_amd.config import RetrievalConfig  # noqa: E402
from audio_rag_amd.retrieval.collection import ChunkCollection  # noqa: E402
from audio_rag_amd.retrieval.device import DenseIndex, SparseIndex  # noqa: E402
from audio_rag_amd.retrieval.mi355x import MI355XRetriever, QueryBatch  # noqa: E402

# (after the package: filter_list_bench puts this tree in front of sys.path, and the modules
# imported above stay those of --package-root)
from filter_list_bench import B, graphed, same, step_ms  # noqa: E402

KEYS = 8
LIVE_TAILS = (1024, 4096)
LIVE_TAIL_ROWS = 2048   # live_tail_rows: a capacity of 4,096 rows holds the larger tail


def payloads(n: int) -> list[dict]:
    """k_j of point i = (i * (2 j + 1) + j) % 8: eight values of n / 8 rows each, per key."""
    cols = [((np.arange(n, dtype=np.int64) * (2 * j + 1) + j) % KEYS).tolist() for j in range(KEYS)]
    return [{"text": "", "metadata": {f"k{j}": cols[j][i] for j in range(KEYS)}} for i in range(n)]


def kernel_ms(slot: int) -> tuple[float, int]:
    total, launches = ctypes.c_double(), ctypes.c_int64()
    _armi.call("armi_kernel_timing_read", slot, ctypes.byref(total), ctypes.byref(launches))
    return total.value, launches.value


def qmask_queries(t) -> int:
    return 0 if t.flags is None else int(((t.flags & _armi.ARMI_FLAG_QMASK) != 0).sum())


def digest(t, mode: str) -> str:
    """sha256 of a result's ids, counts and scores (hybrid: the RRF keys)."""
    sc = t.rank if mode == "hybrid" else t.scores
    h = hashlib.sha256()
    for a in (t.ids, t.count, sc):
        h.update(a.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def live(args, dev) -> None:
    n, dim = args.rows, args.dim
    has_knob = "filter_query_masks_live" in RetrievalConfig.model_fields
    res = {"rows": n, "dim": dim, "batch": B, "steps": args.steps, "rounds": 5,
           "live_tail_rows": LIVE_TAIL_ROWS, "device": torch.cuda.get_device_name(0),
           "filter_rows": n // KEYS, "has_live_knob": has_knob}

    def retriever(live_knob: bool) -> MI355XRetriever:
        kw = {"filter_query_masks_live": True} if live_knob else {}
        return MI355XRetriever(RetrievalConfig(
            filter_query_masks=True, filter_query_masks_sparse=True, live_tail_rows=LIVE_TAIL_ROWS,
            reproduce_sparse_drop=False, query_graphs=False, **kw), dim)

    total = n + max(LIVE_TAILS)
    meta = payloads(total)

    def add(r, lo: int, hi: int) -> None:
        rows = synthetic.make_rows(lo, hi - lo, dim, dev).cpu().numpy()
        ip, ix, iv = (t.cpu().numpy() for t in synthetic.make_sparse_rows(lo, hi - lo, dev))
        ix = ix.astype(np.int32)
        sparse = [(ix[ip[r]:ip[r + 1]], iv[ip[r]:ip[r + 1]]) for r in range(hi - lo)]
        r.add_arrays(rows.view(np.float16), meta[lo:hi], sparse=sparse)

    off = retriever(False)
    for lo in range(0, n, 1 << 17):
        add(off, lo, min(n, lo + (1 << 17)))
    coll = off.collection()
    coll.segments()  # the first build: everything after it goes to the tail
    on = None
    if has_knob:
        on = retriever(True)
        on.attach_collection(coll)
    qd = synthetic.make_queries(1, B, dim, dev, seed=9)[0]
    qi, qx, qv = synthetic.make_sparse_queries(B, dev, seed=10)
    qb = QueryBatch(dense=qd, sparse_indptr=qi, sparse_indices=qx, sparse_values=qv)
    modes = {"dense": 5, "sparse": 20, "hybrid": 20}
    cases = {
        "a_64_distinct_filters": [{f"k{q // KEYS}": q % KEYS} for q in range(B)],
        "b_half_unfiltered_half_one_filter": [None] * (B // 2) + [{"k0": 0}] * (B // 2),
    }

    def search(r, mode, flt):
        return r.search_batch(qb, modes[mode], filter_metadata=flt, search_type=mode)[0]

    at = n
    for tail in LIVE_TAILS:
        add(off, at, n + tail)
        at = n + tail
        seg = coll.segments()
        assert seg.tail is not None and seg.tail.n_rows == tail and seg.main_rows == n, tail
        entry = {}
        for name, flt in cases.items():
            entry[name] = {}
            for mode in modes:
                x = search(off, mode, flt)
                fns = {"off": lambda: search(off, mode, flt)}
                cell = {"digest_off": digest(x, mode),
                        "qmask_groups_off": sum(g.qmask for g in off.last_plan)}
                if on is not None:
                    y = search(on, mode, flt)
                    fns["on"] = lambda: search(on, mode, flt)
                    cell.update(digest_on=digest(y, mode), equal=same(x, y, mode),
                                qmask_groups_on=sum(g.qmask for g in on.last_plan))
                    if mode != "hybrid":
                        cell["qmask_queries_on"] = qmask_queries(y)
                cell.update(step_ms(fns, dev, args.steps, args.warmup, rounds=5))
                entry[name][mode] = cell
        res[f"tail_{tail}"] = entry

    if args.parent_json:
        parent = json.loads(Path(args.parent_json).read_text()).get(str(n), {})
        res["parent"] = {k: v for k, v in parent.items() if k.startswith("tail_")}
        cmp = {}
        for tail in LIVE_TAILS:
            for name in cases:
                for mode in modes:
                    p = parent.get(f"tail_{tail}", {}).get(name, {}).get(mode)
                    c = res[f"tail_{tail}"][name][mode]
                    if not p or "on" not in c:
                        continue
                    spread = max(c["on"]["max_ms"], p["off"]["max_ms"]) - \
                        min(c["on"]["min_ms"], p["off"]["min_ms"])
                    cmp[f"tail_{tail}/{name}/{mode}"] = {
                        "parent_ms": p["off"]["median_ms"], "on_ms": c["on"]["median_ms"],
                        "off_ms": c["off"]["median_ms"],
                        "parent_over_on": p["off"]["median_ms"] / c["on"]["median_ms"],
                        "off_over_parent": c["off"]["median_ms"] / p["off"]["median_ms"],
                        # the two ranges do not overlap: the on step's slowest round is faster
                        # than the parent's fastest
                        "on_beats_parent_beyond_spread": c["on"]["max_ms"] < p["off"]["min_ms"],
                        "rounds_span_ms": spread,
                        "answers_equal": p["digest_off"] == c["digest_on"] == c["digest_off"],
                    }
        res["comparison"] = cmp
    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged[str(n)] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(res))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/filter_masks.json")
    ap.add_argument("--sparse", action="store_true",
                    help="measure filter_query_masks_sparse (sparse and hybrid cells)")
    ap.add_argument("--live", action="store_true",
                    help="measure filter_query_masks_live (a live collection with tail rows)")
    ap.add_argument("--package-root", default=None,
                    help="--live: import audio_rag_amd from this tree (the parent commit's)")
    ap.add_argument("--parent-json", default=None,
                    help="--live: the parent tree's output of this tool, stored under 'parent'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filter_mask_bench needs the GPU")
    dev = torch.device("cuda", 0)
    if args.live:
        return live(args, dev)
    n, dim = args.rows, args.dim
    res = {"rows": n, "dim": dim, "batch": B, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), "filter_rows": n // KEYS}

    dense = DenseIndex(synthetic.make_rows(0, n, dim, dev))
    sparse = SparseIndex(*synthetic.make_sparse_rows(0, n, dev), vocab=synthetic.VOCAB)
    coll = ChunkCollection.from_indexes("audio_rag", dense, payloads(n), sparse)

    def retriever(masks: bool, sparse_masks: bool = False) -> MI355XRetriever:
        r = MI355XRetriever(RetrievalConfig(filter_query_masks=masks,
                                            filter_query_masks_sparse=sparse_masks,
                                            reproduce_sparse_drop=False, query_graphs=False), dim)
        r.attach_collection(coll)
        return r

    off, on = (retriever(True), retriever(True, True)) if args.sparse else \
        (retriever(False), retriever(True))
    qd = synthetic.make_queries(1, B, dim, dev, seed=9)[0]
    qi, qx, qv = synthetic.make_sparse_queries(B, dev, seed=10)
    qb = QueryBatch(dense=qd, sparse_indptr=qi, sparse_indices=qx, sparse_values=qv)
    modes = {"sparse": 20, "hybrid": 20} if args.sparse else {"dense": 5, "hybrid": 20}
    broad = {"k0": 0}
    cases = {
        "a_64_distinct_filters": [{f"k{q // KEYS}": q % KEYS} for q in range(B)],
        "b_half_unfiltered_half_one_filter": [None] * (B // 2) + [broad] * (B // 2),
        "c_one_shared_filter": [broad] * B,
        "d_unfiltered": [None] * B,
    }

    def search(r, mode, flt):
        return r.search_batch(qb, modes[mode], filter_metadata=flt, search_type=mode)[0]

    for name, flt in cases.items():
        entry = {}
        for mode in modes:
            x, y = search(off, mode, flt), search(on, mode, flt)
            entry[mode] = step_ms({"off": lambda: search(off, mode, flt),
                                   "on": lambda: search(on, mode, flt)}, dev, args.steps,
                                  args.warmup)
            entry[mode]["equal"] = same(x, y, mode)
            entry[mode]["qmask_groups"] = sum(g.qmask for g in on.last_plan)
            if mode in ("dense", "sparse"):
                entry[mode]["qmask_queries"] = qmask_queries(y)
        res[name] = entry

    if args.sparse:
        # kernel launch times of the filter scan: one shared mask, (a)'s 64 masks, no mask
        flt = cases["a_64_distinct_filters"]
        k = modes["sparse"]
        one = coll.filter_mask(broad)
        stacked = torch.stack([coll.filter_mask(f) for f in flt])
        qm = torch.arange(B, dtype=torch.int32, device=dev)
        ws = torch.empty(sparse.workspace_bytes(B, k), dtype=torch.uint8, device=dev)
        runs = {"masked_filter_scan": lambda: sparse.topk(qi, qx, qv, k, row_mask=one, workspace=ws),
                "qmask_filter_scan": lambda: sparse.topk_masks(qi, qx, qv, k, stacked, qm,
                                                               workspace=ws),
                "unmasked_filter_scan": lambda: sparse.topk(qi, qx, qv, k, workspace=ws)}
        # (period 2: a sparse call whose whole stage is timed does not time its scan; the two
        # alternate)
        _armi.call("armi_scan_timing_enable", 2)
        kernel_ms(_armi.TIMING_SPARSE_SCAN)
        reps = 10 * args.steps
        times = {}
        for name, fn in runs.items():
            filtered = int(((fn().flags & _armi.ARMI_FLAG_FILTERED) != 0).sum())
            kernel_ms(_armi.TIMING_SPARSE_SCAN)
            for _ in range(reps):
                fn()
            total, launches = kernel_ms(_armi.TIMING_SPARSE_SCAN)
            kernel_ms(_armi.TIMING_SPARSE_STAGE)
            times[name] = total / max(launches, 1)
            times[name + "_launches"] = launches
            times[name + "_filtered_queries"] = filtered
        _armi.call("armi_scan_timing_enable", 0)
        times["qmask_over_masked_scan"] = times["qmask_filter_scan"] / times["masked_filter_scan"]
        res["kernels_ms"] = times
        out = Path(args.out)
        merged = json.loads(out.read_text()) if out.exists() else {}
        merged[str(n)] = res
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(merged, indent=1) + "\n")
        print(json.dumps(res))
        return

    # the dense legs of (a) and (b) as device work only, replayed from HIP graphs
    k = modes["dense"]
    for name in ("a_64_distinct_filters", "b_half_unfiltered_half_one_filter"):
        flt = cases[name]
        distinct = []
        for f in flt:
            if f not in distinct:
                distinct.append(f)
        subs = [(qd[[i for i, qf in enumerate(flt) if qf == f]].contiguous(), coll.filter_mask(f))
                for f in distinct]
        ws = torch.empty(dense.workspace_bytes(B, k), dtype=torch.uint8, device=dev)
        real = [f for f in distinct if f]
        stacked = torch.stack([coll.filter_mask(f) for f in real])
        qm = torch.tensor([real.index(f) if f else -1 for f in flt], dtype=torch.int32, device=dev)
        wsq = torch.empty(dense.qmask_workspace_bytes(B, k, len(real)), dtype=torch.uint8,
                          device=dev)
        g_off = graphed(lambda: [dense.topk(q, k, row_mask=m, workspace=ws) for q, m in subs][-1],
                        dev)
        g_on = graphed(lambda: dense.topk_masks(qd, k, stacked, qm, workspace=wsq), dev)
        if g_off is not None and g_on is not None:
            res[name]["dense"]["graph"] = step_ms({"off": g_off, "on": g_on}, dev, args.steps,
                                                  args.warmup)
        if name == "a_64_distinct_filters":
            # kernel launch times: the qmask scan and its mask image against the plain masked scan
            one = coll.filter_mask(broad)
            _armi.call("armi_scan_timing_enable", 1)
            kernel_ms(_armi.TIMING_DENSE_SCAN), kernel_ms(_armi.TIMING_QMASK_PREP)
            reps = 5 * args.steps
            for _ in range(reps):
                dense.topk(qd, k, row_mask=one, workspace=ws)
            plain = kernel_ms(_armi.TIMING_DENSE_SCAN)
            for _ in range(reps):
                dense.topk_masks(qd, k, stacked, qm, workspace=wsq)
            scan, prep = kernel_ms(_armi.TIMING_DENSE_SCAN), kernel_ms(_armi.TIMING_QMASK_PREP)
            _armi.call("armi_scan_timing_enable", 0)
            res["kernels_ms"] = {
                "masked_int8_scan": plain[0] / max(plain[1], 1),
                "qmask_int8_scan": scan[0] / max(scan[1], 1),
                "qmask_prep": prep[0] / max(prep[1], 1),
                "launches": [plain[1], scan[1], prep[1]],
                "qmask_over_masked_scan": (scan[0] / max(scan[1], 1)) / (plain[0] / max(plain[1], 1)),
            }

    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged[str(n)] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
