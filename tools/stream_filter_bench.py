#!/usr/bin/env python
"""Mixed-filter traffic through the native StreamServer: what
StreamServer(query_masks=True) buys requests that each bring their own payload filter.

One hybrid collection of --rows x --dim synthetic points with eight metadata keys k0..k7 of eight
values each (filter_mask_bench.py's: every filter {k_j: v} matches rows / 8), one server per arm
with max_batch 64. The server is driven in windows: submit W = 64 tickets from one thread, wait
for all 64, repeat; a window's time is the host clock from its first submit to its last wait.
Only armi_stream_submit_ex / armi_stream_wait are called, with every query, term array and mask
pointer prepared ahead, so the same file runs on a checkout of the parent commit, whose
StreamServer has no query_masks keyword (--package-root DIR imports that tree, which gives the
flag-off arm only).

  workloads  a: 64 distinct broad filters (rows / 8 rows each)
             b: 32 unfiltered + 32 under one broad filter
             d: 64 unfiltered
  modes      dense top-5, hybrid 40 + 40 -> 20

Per arm (--label, e.g. on / off / parent_1 / parent_2) and cell: the median, min, max and
interquartile range of --windows windows after --warmup, the batches and mixed batches the
windows made, and a sha256 of the last window's ids and counts (the arms must agree). The result
is merged into --out under the label.

    python tools/stream_filter_bench.py --label on --query-masks 1 --commit abc1234
    python tools/stream_filter_bench.py --label off --query-masks 0 --commit abc1234
    python tools/stream_filter_bench.py --label parent_1 --package-root ../parent --commit def5678
"""

from __future__ import annotations

import argparse
import ctypes
import hashlib
import inspect
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

# (--package-root is read before the package is imported)
_root = [a.split("=", 1)[1] if "=" in a else sys.argv[i + 1] for i, a in enumerate(sys.argv)
         if a == "--package-root" or a.startswith("--package-root=")]
ROOT = Path(_root[0]).resolve() if _root else Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from audio_rag_amd import _armi, synthetic  # noqa: E402
from audio_rag_amd.config import RetrievalConfig  # noqa: E402
from audio_rag_amd.retrieval.batcher import StreamServer  # noqa: E402
from audio_rag_amd.retrieval.collection import ChunkCollection  # noqa: E402
from audio_rag_amd.retrieval.device import DenseIndex, SparseIndex  # noqa: E402
from audio_rag_amd.retrieval.mi355x import MI355XRetriever  # noqa: E402

W = 64
KEYS = 8
MODES = {"dense": 5, "hybrid": 20}


def payloads(n: int) -> list[dict]:
    """k_j of point i = (i * (2 j + 1) + j) % 8: eight values of n / 8 rows each, per key."""
    cols = [((np.arange(n, dtype=np.int64) * (2 * j + 1) + j) % KEYS).tolist() for j in range(KEYS)]
    return [{"text": "", "metadata": {f"k{j}": cols[j][i] for j in range(KEYS)}} for i in range(n)]


def commit_of(root: Path) -> str:
    try:
        return subprocess.run(["git", "-C", str(root), "rev-parse", "--short", "HEAD"],
                              capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def window(srv, handle, qptr, sp, masks, mode_code, out) -> float:
    """One window: W submits, W waits. Returns its time in ms; out receives ids and counts."""
    call = _armi.call
    ticket = ctypes.c_int64()
    tickets = [0] * W
    count, mode = ctypes.c_int32(), ctypes.c_int32()
    ids, cnt = out
    t0 = time.perf_counter()
    for i in range(W):
        call("armi_stream_submit_ex", handle, qptr[i], sp[i][0], sp[i][1], sp[i][2], mode_code,
             masks[i], ctypes.byref(ticket))
        tickets[i] = ticket.value
    for i in range(W):
        call("armi_stream_wait", handle, tickets[i], None, ids[i].ctypes.data, None,
             ctypes.byref(count), ctypes.byref(mode), 60e6)
        cnt[i] = count.value
    return (time.perf_counter() - t0) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-wait-ms", type=float, default=2.0)
    ap.add_argument("--query-masks", type=int, default=1)
    ap.add_argument("--label", required=True)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--out", default="profiles/stream_query_masks.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_filter_bench needs the GPU")
    if args.windows < 20:
        raise SystemExit("at least 20 windows per cell")
    dev = torch.device("cuda", 0)
    n, dim = args.rows, args.dim
    has_flag = "query_masks" in inspect.signature(StreamServer.__init__).parameters
    flag = bool(args.query_masks) and has_flag
    res = {"commit": args.commit or commit_of(ROOT), "rows": n, "dim": dim, "window": W,
           "windows": args.windows, "warmup": args.warmup, "max_batch": W,
           "max_wait_ms": args.max_wait_ms, "query_masks": flag, "has_flag": has_flag,
           "device": torch.cuda.get_device_name(0), "filter_rows": n // KEYS, "cells": {}}

    dense = DenseIndex(synthetic.make_rows(0, n, dim, dev))
    sparse = SparseIndex(*synthetic.make_sparse_rows(0, n, dev), vocab=synthetic.VOCAB)
    coll = ChunkCollection.from_indexes("audio_rag", dense, payloads(n), sparse)
    ret = MI355XRetriever(RetrievalConfig(reproduce_sparse_drop=False, query_graphs=False), dim)
    ret.attach_collection(coll)

    qd = synthetic.make_queries(1, W, dim, dev, seed=9)[0].cpu().numpy()
    qd = np.ascontiguousarray(qd.view(np.float16) if qd.dtype != np.float16 else qd)
    qi, qx, qv = (t.cpu().numpy() for t in synthetic.make_sparse_queries(W, dev, seed=10))
    qx, qv = np.ascontiguousarray(qx, np.int32), np.ascontiguousarray(qv, np.float32)
    qptr = [qd[i].ctypes.data for i in range(W)]
    terms = [(qx[qi[i]:].ctypes.data, qv[qi[i]:].ctypes.data, int(qi[i + 1] - qi[i]))
             for i in range(W)]
    none = [(None, None, 0)] * W
    broad = {"k0": 0}
    workloads = {
        "a_64_distinct_filters": [{f"k{q // KEYS}": q % KEYS} for q in range(W)],
        "b_half_unfiltered_half_one_filter": [None] * (W // 2) + [broad] * (W // 2),
        "d_unfiltered": [None] * W,
    }

    for mode, k in MODES.items():
        kw = {"query_masks": True} if flag else {}
        with StreamServer(ret, top_k=k, max_batch=W, max_wait_ms=args.max_wait_ms,
                          search_type=mode, **kw) as srv:
            handle = srv._handle
            ids = np.empty((W, k), dtype=np.int64)
            cnt = np.empty(W, dtype=np.int32)
            for name, flt in workloads.items():
                held = [coll.filter_mask(f) for f in flt]      # alive for the whole cell
                masks = [None if m is None else m.data_ptr() for m in held]
                sp = terms if mode == "hybrid" else none
                code = 0 if mode == "hybrid" else 1            # ARMI_STREAM_AUTO / _DENSE
                for _ in range(args.warmup):
                    window(srv, handle, qptr, sp, masks, code, (ids, cnt))
                b0 = srv.stats_ex() if has_flag else srv.stats() + (0,)
                ms = [window(srv, handle, qptr, sp, masks, code, (ids, cnt))
                      for _ in range(args.windows)]
                b1 = srv.stats_ex() if has_flag else srv.stats() + (0,)
                a = np.asarray(ms)
                h = hashlib.sha256()
                h.update(ids.tobytes())
                h.update(cnt.tobytes())
                res["cells"][f"{name}/{mode}"] = {
                    "median_ms": float(np.median(a)), "min_ms": float(a.min()),
                    "max_ms": float(a.max()),
                    "iqr_ms": float(np.percentile(a, 75) - np.percentile(a, 25)),
                    "windows_ms": [round(float(x), 4) for x in a],
                    "batches": b1[0] - b0[0], "queries": b1[1] - b0[1],
                    "mixed_batches": b1[2] - b0[2], "digest": h.hexdigest()[:16]}
                del held

    out = Path(args.out)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged[args.label] = res
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(merged, indent=1) + "\n")
    print(json.dumps({kk: {f: v[f] for f in ("median_ms", "min_ms", "max_ms", "batches",
                                             "mixed_batches", "digest")}
                      for kk, v in res["cells"].items()}))


if __name__ == "__main__":
    main()
