"""Benchmark of the MI355X retrieval hot path (BASELINE.json metric).

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run does only what the headline needs: set-up, W warm-up steps, the K timed steps, the
outputs of the last timed step as .npy files when --dump-outputs is given, and the result line
(the scan's roofline rides on event pairs recorded inside the timed steps). --full adds everything
else the line can carry: step and single-query p50 latencies, certified_frac, the sparse stage's
rooflines (re-runs of its kernels alone), the cpu_baseline and the secondary configurations
(configs1 / configs2 / size sweep / hybrid / pipeline / configs3_rank, each a child run).

Workload (BASELINE.json metric "queries/sec + p50 latency, 1M x 1024-d chunks, top-5"):
  a 1M x 1024 fp16 chunk store (synthetic unit vectors) sharded by chunk
  ordinal over the N GPUs; every step each GPU brings its own batch of 64 queries; a step is
    all-gather queries (RCCL) -> armi_dense_topk of all N*64 queries on the local shard ->
    all-gather the per-shard top-5 (RCCL) -> armi_topk_merge_shards of this GPU's 64 queries.
  At N=1 the collectives vanish. Per-GPU work is fixed (shard rows x N*64 queries = 1M x 64),
  so scaling is weak; value = all queries answered by all GPUs / time.
Inputs are resident in HBM before the timed region; the timed region is K steps bracketed by a
barrier + synchronize on both sides, max over ranks.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

from audio_rag_amd.synthetic import (VOCAB, doc_tokens, make_clustered_queries,  # noqa: E402
                                     make_clustered_rows, make_queries, make_rows,
                                     make_sparse_queries, make_sparse_rows)

METRIC = json.loads((ROOT / "BASELINE.json").read_text())["metric"]
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md chip table)
# dense (non-sparse) matrix peaks, MI355X_MICROARCH.md: bf16/f16 ~2.5 PF; fp32-input MFMA runs at
# 1/16 of the bf16 rate (cdna_hip_programming.md §3 'FP32-input MFMA')
MFMA_PEAK_TFLOPS = {"fp16": 2500.0, "bf16": 2500.0, "fp32": 157.0, "i8": 5000.0}  # dense, no sparsity

# measured fp16 MFMA ceiling under the chip's clock management (back-to-back MFMAs on random
# operands hold ~1.63 GHz, not 2.4): profiles/r02o_mfma_ceiling.txt; reported beside the spec peak
MFMA_PRACTICAL_TFLOPS = {"fp16": 1674.0}


def cpu_model() -> str:
    try:
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


class CpuReference:
    """The reference's CPU search path, restated in numpy / scipy / transformers on the host
    cores of the GPU box (bench.py's cpu_baseline leg; oracle/ is the checker, this is timing).

    What the reference runs per query with an in-process Qdrant (qdrant-client local mode,
    configs/development.yaml `qdrant_in_memory: true`), QdrantRetriever.search
    (src/audio_rag/retrieval/qdrant.py:227-352):
      * dense COSINE: vectors normalised in fp32 at insert, query normalised, fp32 dot over every
        stored vector, full argsort of the score vector, first `limit` (qdrant.py:316-323);
      * hybrid: the dense prefetch (limit 2k) and the sparse prefetch (limit 2k: dot over the
        rows sharing a term with the query) fused by RRF 1/(2+pos) in python floats
        (qdrant.py:281-298; oracle.rrf);
      * rerank: sentence-transformers CrossEncoder.predict = XLMRobertaForSequenceClassification
        fp32 forward of the (query, chunk) pairs + sigmoid (reranking/bge.py:119-123), here the
        transformers model with the bench's seeded weights.
    The sparse prefetch uses a column-gathered CSC product (scipy), which is faster than local
    mode's per-point loop: the baseline is generous to the CPU, never the other way round.
    Two modes: "reference-shaped" (one query per call, as AudioRAG.query() issues them; p50 and
    queries / s over >= `min_queries` queries or the time budget) and "batched" (B = 64 queries
    per numpy GEMM, labelled separately)."""

    def __init__(self, rows_dev: torch.Tensor, csr_dev=None, threads: int | None = None):
        self.threads = threads or int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
        torch.set_num_threads(self.threads)
        x = rows_dev.float()
        # qdrant COSINE normalises at insert (fp32), off the clock; done on the device for speed
        self.x = (x / x.norm(dim=1, keepdim=True)).cpu().numpy()
        del x
        self.csc = None
        if csr_dev is not None:
            import scipy.sparse as sp
            indptr, indices, values = (t.cpu().numpy() for t in csr_dev)
            self.csc = sp.csr_matrix((values, indices, indptr),
                                     shape=(indptr.size - 1, VOCAB)).tocsc()

    @staticmethod
    def _unit(q: np.ndarray) -> np.ndarray:
        q = q.astype(np.float32)
        return q / np.linalg.norm(q, axis=-1, keepdims=True)

    def dense_one(self, q: np.ndarray, limit: int) -> np.ndarray:
        s = self.x @ self._unit(q)
        return np.argsort(s)[::-1][:limit]

    def sparse_one(self, qi: np.ndarray, qv: np.ndarray, limit: int) -> np.ndarray:
        sub = self.csc[:, qi]
        s = sub @ qv.astype(np.float32)
        cand = np.unique(sub.indices)
        order = np.argsort(-s[cand], kind="stable")[:limit]
        return cand[order]

    def hybrid_one(self, q, qi, qv, limit: int) -> list:
        from oracle import oracle
        d = self.dense_one(q, 2 * limit).tolist()
        s = self.sparse_one(qi, qv, 2 * limit).tolist()
        return oracle.rrf([d, s], limit)

    def dense_batch(self, qb: np.ndarray, limit: int) -> np.ndarray:
        s = self._unit(qb) @ self.x.T
        part = np.argpartition(-s, limit, axis=1)[:, :limit]
        return np.take_along_axis(part, np.argsort(-np.take_along_axis(s, part, 1), 1), 1)

    def hybrid_batch(self, qb, q_csr, limit: int) -> list:
        import scipy.sparse as sp
        from oracle import oracle
        d = self.dense_batch(qb, 2 * limit)
        qp, qi, qv = q_csr
        qm = sp.csr_matrix((qv.astype(np.float32), qi, qp), shape=(qp.size - 1, VOCAB))
        s = (qm @ self.csc.T).tocsr()  # [B, N] sparse: only rows sharing a term
        out = []
        for b in range(qb.shape[0]):
            row = s.getrow(b)
            order = np.argsort(-row.data, kind="stable")[:2 * limit]
            out.append(oracle.rrf([d[b].tolist(), row.indices[order].tolist()], limit))
        return out


def time_calls(fn, items: list, min_calls: int, budget_s: float) -> tuple[list[float], int]:
    """Per-call wall times of fn(item) cycling over items: at least min_calls calls unless the
    budget runs out first, after one warm-up call."""
    fn(items[0])
    lat = []
    t0 = time.perf_counter()
    while len(lat) < min_calls and time.perf_counter() - t0 < budget_s:
        it = items[len(lat) % len(items)]
        t = time.perf_counter()
        fn(it)
        lat.append(time.perf_counter() - t)
    return lat, len(lat)


def cpu_baseline(wl: str, ref: CpuReference, queries: np.ndarray, q_csr: list | None, k: int,
                 search_k: int, rerank_pairs=None, budget_s: float = 40.0) -> dict:
    """cpu_baseline object of the bench line: the reference-shaped single-query mode is `value`,
    the batched B = 64 mode rides along under "batched"."""
    from threadpoolctl import threadpool_limits

    nq = queries.shape[0]
    with threadpool_limits(limits=ref.threads):
        if wl == "dense":
            one = lambda i: ref.dense_one(queries[i], k)
            batch = lambda j: ref.dense_batch(queries[64 * j:64 * (j + 1)], k)
            what = f"dense COSINE top-{k}: fp32 dot over all rows + full argsort"
        else:
            one = lambda i: ref.hybrid_one(queries[i], q_csr[i][0], q_csr[i][1], search_k)
            batch = lambda j: ref.hybrid_batch(queries[64 * j:64 * (j + 1)], q_csr_batch[j], search_k)
            what = (f"hybrid: dense prefetch {2 * search_k} (fp32 dot + full argsort) + sparse "
                    f"prefetch {2 * search_k} (CSC column gather) -> python RRF -> {search_k}")
            q_csr_batch = []
            for j in range(nq // 64):
                parts = q_csr[64 * j:64 * (j + 1)]
                qp = np.zeros(65, dtype=np.int64)
                qp[1:] = np.cumsum([p[0].size for p in parts])
                q_csr_batch.append((qp, np.concatenate([p[0] for p in parts]),
                                    np.concatenate([p[1] for p in parts])))
        lat, n_one = time_calls(one, list(range(nq)), 200, budget_s)
        blat, n_b = time_calls(batch, list(range(max(nq // 64, 1))), 4, budget_s / 3)
        p50 = statistics.median(lat)
        rr = None
        if rerank_pairs is not None:
            model, pairs = rerank_pairs  # transformers model (CPU fp32), [q, 20, L] int64 ids

            @torch.inference_mode()
            def rerank_one(i):
                ids = pairs[i]
                return torch.sigmoid(model(input_ids=ids, attention_mask=torch.ones_like(ids)).logits)

            rlat, n_r = time_calls(rerank_one, list(range(pairs.shape[0])), 5, budget_s)
            rr = {"p50_ms": statistics.median(rlat) * 1e3, "queries": n_r,
                  "pairs_per_query": int(pairs.shape[1]), "seq_len": int(pairs.shape[2])}
            p50 += statistics.median(rlat)
            what += (f" -> cross-encoder fp32 (transformers XLM-R base, {pairs.shape[1]} pairs x "
                     f"{pairs.shape[2]} tokens) + sigmoid + stable sort -> top-{k}")
    res = {
        "value": 1.0 / p50,
        "unit": "queries/sec",
        "cores": ref.threads,
        "host_cores": os.cpu_count(),
        "cores_note": (f"{ref.threads} threads used (the box's OMP_NUM_THREADS share) on a host "
                       f"with {os.cpu_count()} logical CPUs"),
        "kind": "port",
        "mode": "reference-shaped: one query per call, as AudioRAG.query() issues it",
        "p50_ms": p50 * 1e3,
        "sample": (f"{what}; qdrant-client local-mode arithmetic restated in numpy over all "
                   f"{ref.x.shape[0]} rows; {n_one} single-query searches, value = 1 / p50"
                   + (f"; rerank p50 over {rr['queries']} queries added" if rr else "")),
        "cpu_model": cpu_model(),
        "batched": {"value": 64 * n_b / sum(blat), "unit": "queries/sec", "batch": 64,
                    "batches": n_b, "sample": ("the same search arithmetic, 64 queries per numpy "
                                               "GEMM (argpartition selection)"
                                               + ("; search only, the rerank is not in this mode"
                                                  if rr else ""))},
    }
    if rr:
        res["rerank"] = rr
    return res


TRAFFIC_DIR = ROOT / "profiles" / "traffic"


def traffic_key(form: int, n_rows: int, dim: int, n_queries: int, corpus: str) -> str:
    """Name of the committed PMC measurement of one scan shape (tools/pmc_dense_traffic.sh)."""
    name = {0: "fp16", 1: "i8", 2: "tiled", 3: "tiled_i8"}.get(form, f"form{form}")
    return f"dense_{name}_{corpus}_n{n_rows}_d{dim}_q{n_queries}"


def read_traffic(key: str, kernel: str) -> tuple[float | None, str | None]:
    """HBM bytes per launch of the scan measured by rocprofv3 PMC passes (FETCH_SIZE and
    WRITE_SIZE in separate runs, gfx950-corrected) for exactly this shape and kernel instance, or
    (None, None) when no such measurement is committed: a traffic figure of another shape or
    kernel says nothing here."""
    p = TRAFFIC_DIR / f"{key}.json"
    if not p.exists():
        return None, None
    try:
        d = json.loads(p.read_text())
        if d.get("key") != key or d.get("kernel") != kernel:
            return None, None
        return float(d["hbm_bytes_per_launch"]), str(p.relative_to(ROOT))
    except Exception:
        return None, None


def dump_outputs(out_dir: Path, top) -> None:
    """--dump-outputs: the TopK the last timed step returned, one DIR/<name>.npy per field.
    scores stay float32; ids, rank, count and flags are written as float64 (exact for chunk
    ordinals and flag bits). The inputs are seeded, so two builds run with the same arguments can
    be compared file by file."""
    out_dir.mkdir(parents=True, exist_ok=True)
    fields = {"scores": (top.scores, np.float32), "ids": (top.ids, np.float64),
              "rank": (top.rank, np.float64), "count": (top.count, np.float64),
              "flags": (top.flags, np.float64)}
    torch.cuda.synchronize()
    for name, (t, dtype) in fields.items():
        if t is not None:
            np.save(out_dir / f"{name}.npy", t.detach().cpu().numpy().astype(dtype))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: p50 latencies, certified_frac, the sparse stage's "
                         "rooflines, the cpu_baseline and the secondary configurations (child "
                         "runs); --no-cpu-baseline / --no-extras / --latency-iters trim those")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (scores, ids, rank, count, "
                         "flags of its TopK) as DIR/<name>.npy, float32 / float64")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--eager-hybrid", action="store_true",
                    help="hybrid workloads: launch each step's kernels from Python instead of "
                         "replaying the step's HIP graph (retrieval.device.HybridGraph)")
    ap.add_argument("--no-extras", action="store_true",
                    help="dense headline at N=1 only: skip the secondary configs1 / configs2 "
                         "objects (each measured by a child bench.py run)")
    ap.add_argument("--latency-iters", type=int, default=30)
    ap.add_argument("--cpu-budget", type=float, default=20.0,
                    help="seconds per timed leg of the cpu_baseline (single-query, batched, rerank)")
    ap.add_argument("--workload", choices=["dense", "hybrid", "hybrid_rerank", "stream", "pipeline",
                                           "ingest"],
                    default="dense",
                    help="dense: BASELINE metric (default); hybrid: dense+sparse prefetch 2k + RRF "
                         "(configs[2] without rerank); hybrid_rerank: configs[2]: top-20 fused -> "
                         "cross-encoder -> top-k; stream: single queries arriving at --qps "
                         "(Poisson) through QueryBatcher -> MI355XRetriever, reference-shaped "
                         "results (configs[4]'s streaming query, 1 GPU); pipeline: "
                         "QueryPipeline.query() one query at a time (BGE-M3 encode -> hybrid "
                         "search -> rerank), per-stage latency beside the reference's published "
                         "numbers")
    ap.add_argument("--corpus", choices=["random", "clustered"], default="random",
                    help="random: isotropic unit rows (SURVEY §8(d)); clustered: anisotropic "
                         "lecture corpus (shared mean direction, topics, overlapping-chunk runs "
                         "of near-duplicate ordinals, exact re-uploads; synthetic.py) with "
                         "queries near random chunks")
    ap.add_argument("--queries", type=int, default=200, help="pipeline: timed queries")
    ap.add_argument("--qps", type=float, default=20000.0, help="stream: offered queries/s")
    ap.add_argument("--duration", type=float, default=4.0, help="stream: seconds of arrivals")
    ap.add_argument("--stream-front", choices=["native", "python"], default="native",
                    help="stream: native StreamServer + native load generator, or a Python "
                         "client through QueryBatcher")
    ap.add_argument("--max-wait-ms", type=float, default=2.0, help="stream: batching window")
    ap.add_argument("--ingest-chunks", type=int, default=20000, help="ingest: chunks embedded")
    ap.add_argument("--max-batch", type=int, default=64,
                    help="stream (native): largest batch the server coalesces")
    ap.add_argument("--search-type", choices=["dense", "hybrid"], default="dense",
                    help="stream: dense top-k, or hybrid (dense + sparse prefetch 2k, RRF)")
    ap.add_argument("--initial-k", type=int, default=20)
    ap.add_argument("--rerank-dtype", choices=["fp32", "bf16", "fp16"], default="fp16",
                    help="cross-encoder GEMM dtype (fp16: fp16 GEMMs + fused fp16 attention, "
                         "within the 1e-3 score budget; fp32: the reference's dtype)")
    args = ap.parse_args()

    if args.workload == "stream":
        return stream_main(args)
    if args.workload == "pipeline":
        return pipeline_main(args)
    if args.workload == "ingest":
        return ingest_main(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print(f"warning: --gpus {args.gpus} but WORLD_SIZE {world}; using {world}", file=sys.stderr)
    # ARMI_BENCH_BACKEND=gloo rehearses the N>1 path with several ranks sharing the GPUs of a
    # smaller box (RCCL refuses two ranks on one device); the driver's runs use RCCL
    backend = os.environ.get("ARMI_BENCH_BACKEND", "nccl")
    gpu = local_rank % max(torch.cuda.device_count(), 1) if backend == "gloo" else local_rank
    torch.cuda.set_device(gpu)
    dev = torch.device("cuda", gpu)
    # ARMI_BENCH_SHARDED=1 runs the sharded step (collectives, merge) even at WORLD_SIZE 1: the
    # exchange's own cost on one GPU, without any link latency
    distributed = world > 1 or os.environ.get("ARMI_BENCH_SHARDED") == "1"
    if distributed:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from audio_rag_amd import _armi
    from audio_rag_amd.retrieval.device import (ConcurrentHybrid, DenseIndex, HybridGraph,
                                                SparseIndex, TopK, merge_shards,
                                                merge_shards_packed, rrf_fuse)
    from audio_rag_amd.retrieval.shards import ShardedSearch, shard_range

    n, dim, batch, k = args.chunks, args.dim, args.batch, args.top_k
    wl = args.workload
    # hybrid and hybrid_rerank search configs[2]'s shape: top initial_k (20) fused from dense +
    # sparse prefetches of 2 * 20 (QueryPipeline.query -> search(top_k=20), qdrant.py:281-298)
    search_k = k if wl == "dense" else args.initial_k
    pre_k = search_k if wl == "dense" else 2 * search_k
    lo, hi = shard_range(n, rank, world)
    n_q_batches = 8
    if args.corpus == "clustered":
        rows = make_clustered_rows(lo, hi - lo, dim, dev)
        queries = make_clustered_queries(n_q_batches * batch, n, dim, dev,
                                         seed=1 + rank).view(n_q_batches, batch, dim)
    else:
        rows = make_rows(lo, hi - lo, dim, dev)
        queries = make_queries(n_q_batches, batch, dim, dev, seed=1 + rank)
    index = DenseIndex(rows, ordinal_base=lo)
    ws = torch.empty(index.workspace_bytes(world * batch, pre_k), dtype=torch.uint8, device=dev)
    sindex = None
    hgraph = hg_batches = None
    q_sparse = []
    csr = None
    if wl != "dense":
        csr = make_sparse_rows(lo, hi - lo, dev)
        sindex = SparseIndex(*csr, vocab=VOCAB, ordinal_base=lo)
        sws = torch.empty(sindex.workspace_bytes(world * batch, pre_k), dtype=torch.uint8, device=dev)
        q_sparse = [make_sparse_queries(batch, dev, seed=1000 * (1 + rank) + j) for j in range(n_q_batches)]
        hybrid = ConcurrentHybrid(dev)
        # the full-batch step replays a HIP graph of the same kernels (launch overhead off the
        # GPU's critical path); the single-query latency probe stays eager
        hgraph = (HybridGraph(index, sindex, batch, pre_k, search_k)
                  if not distributed and not args.eager_hybrid else None)
        # each batch arrives as one staging buffer (as a request would): one copy per step
        hg_batches = ([hgraph.pack(queries[j], *q_sparse[j]) for j in range(n_q_batches)]
                      if hgraph is not None else None)
    reranker = None
    hf_reranker = None
    if wl == "hybrid_rerank":
        from audio_rag_amd.reranking.xlmr import CrossEncoderXLMR, build_reranker
        hf_reranker = build_reranker(seed=5)
        reranker = CrossEncoderXLMR(hf_reranker, dev)
        if args.rerank_dtype != "fp32":
            reranker.to_dtype({"bf16": torch.bfloat16, "fp16": torch.float16}[args.rerank_dtype])
        gq = torch.Generator(device=dev).manual_seed(4 + rank)
        q_tokens = torch.randint(4, VOCAB, (n_q_batches, batch, 16), generator=gq, device=dev,
                                 dtype=torch.int32)
    sharded = None
    if distributed:
        sharded = ShardedSearch(lambda q, kk: index.topk(q, kk, workspace=ws), merge_shards,
                                local_sparse=(lambda c, kk: sindex.topk(*c, kk, workspace=sws)) if sindex else None,
                                rrf=lambda a, b, kk: rrf_fuse(a, b, kk),
                                merge_packed=merge_shards_packed)

    # live timing of the cross-encoder forward (runs on torch's current stream)
    rr_timing = {"on": False, "events": [], "flops": 0.0}

    def rerank(fused: TopK, qt: torch.Tensor) -> TopK:
        """configs[2]: every query's fused candidates -> (query, chunk) pairs of L = 256 tokens
        (<s> q16 </s></s> d236 </s>) -> cross-encoder -> stable sort -> top-k."""
        nb, kc = fused.ids.shape
        ids = fused.ids.clamp(min=0)
        d = doc_tokens(ids, 236)
        eos = torch.full((nb, kc, 1), 2, dtype=torch.int32, device=dev)
        bos = torch.zeros((nb, kc, 1), dtype=torch.int32, device=dev)
        qq = qt[:, None, :].expand(nb, kc, qt.shape[1])
        pairs = torch.cat([bos, qq, eos, eos, d, eos], dim=2).reshape(nb * kc, -1).contiguous()
        valid = (torch.arange(kc, device=dev)[None, :] < fused.count[:, None])
        mask = torch.ones_like(pairs)
        if rr_timing["on"]:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        probs = reranker.forward(pairs, mask).view(nb, kc)
        if rr_timing["on"]:
            ev[1].record()
            rr_timing["events"].append(ev)
            rr_timing["flops"] += reranker.flops(pairs.shape[0], pairs.shape[1])
        probs = torch.where(valid, probs, torch.full_like(probs, -1.0))
        order = torch.sort(probs, dim=1, descending=True, stable=True).indices[:, :k]
        return TopK(scores=torch.gather(probs, 1, order), ids=torch.gather(fused.ids, 1, order),
                    rank=torch.gather(probs, 1, order).double(),
                    count=torch.clamp(fused.count, max=k))

    def step(i: int, q_local: torch.Tensor | None = None):
        j = i % n_q_batches
        ql = q_local if q_local is not None else queries[j]
        if wl == "dense":
            if sharded is None:
                return index.topk(ql, k, workspace=ws)
            return sharded.dense(ql, k)
        qs = q_sparse[j]
        if ql.shape[0] != batch:  # single-query latency probe
            qs = (qs[0][:ql.shape[0] + 1], qs[1], qs[2])
        if sharded is None and hgraph is not None and q_local is None:
            fused = hgraph(hg_batches[j])
        elif sharded is None and hgraph is not None and ql.shape[0] == batch:
            fused = hgraph(ql, *qs)
        elif sharded is None:
            fused = hybrid(lambda: index.topk(ql, pre_k, workspace=ws),
                           lambda: sindex.topk(*qs, pre_k, workspace=sws), qs, search_k)
        else:
            fused = sharded.hybrid(ql, qs, search_k)
        if reranker is None:
            return fused
        return rerank(fused, q_tokens[j][:ql.shape[0]])

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        step(i)
    barrier()
    # every 8th launch of the timed kernels carries its event pair (an event-bound dispatch costs
    # ~5 us of a 61-us step at 100k rows; profiles/r06_timing_cost_ab.txt); ARMI_BENCH_TIMING
    # overrides the period (0 = off, for that A/B)
    _armi.call("armi_scan_timing_enable", int(os.environ.get("ARMI_BENCH_TIMING", "8")))
    for slot in (_armi.TIMING_DENSE_SCAN, _armi.TIMING_SPARSE_SCAN, _armi.TIMING_SPARSE_STAGE):
        _armi.call("armi_kernel_timing_read", slot, _armi.ctypes.byref(_armi.ctypes.c_double()),
                   _armi.ctypes.byref(_armi.ctypes.c_int64()))
    barrier()
    rr_timing["on"] = reranker is not None
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = step(i)
    barrier()
    elapsed = time.perf_counter() - t0
    rr_timing["on"] = False
    if args.dump_outputs and rank == 0 and last is not None:
        dump_outputs(Path(args.dump_outputs), last)
    full = args.full
    scan_timing_note = None
    if full and wl != "dense" and hgraph is not None:
        # The timed steps replayed the step's HIP graph, whose launches record no host-side HIP
        # events: the scans' launch times come from eager launches of the same kernels over the
        # same batches right after the timed region (the rerank, timed above, is not rerun).
        n_eager = min(args.steps, 20)
        # (outside the timed region: every launch; period 2 so that a sparse call times either
        # its whole stage or its scan, never both)
        _armi.call("armi_scan_timing_enable", 2 if sindex is not None else 1)
        for i in range(n_eager):
            j = i % n_q_batches
            hybrid(lambda: index.topk(queries[j], pre_k, workspace=ws),
                   lambda: sindex.topk(*q_sparse[j], pre_k, workspace=sws), q_sparse[j], search_k)
        barrier()
        scan_timing_note = (f"scan launch times from {n_eager} eager hybrid steps of the same "
                            "batches after the timed region (the timed steps replay a HIP graph)")
    sparse_timing = {}
    if full and wl != "dense" and sindex is not None and world == 1:
        # the sparse stage inside the step shares the GPU with the dense scan (two streams); its
        # own duration: the same calls alone on the stream, right after
        for slot, key in ((_armi.TIMING_SPARSE_SCAN, "scan_in_step"),
                          (_armi.TIMING_SPARSE_STAGE, "stage_in_step")):
            v, c = _armi.ctypes.c_double(), _armi.ctypes.c_int64()
            _armi.call("armi_kernel_timing_read", slot, _armi.ctypes.byref(v), _armi.ctypes.byref(c))
            sparse_timing[key] = (v.value, c.value)
        barrier()
        _armi.call("armi_scan_timing_enable", 2)  # stage and scan timed on alternate calls
        for i in range(max(min(args.steps, 40), 8)):
            sindex.topk(*q_sparse[i % n_q_batches], pre_k, workspace=sws)
        barrier()
        for slot, key in ((_armi.TIMING_SPARSE_SCAN, "scan_alone"),
                          (_armi.TIMING_SPARSE_STAGE, "stage_alone")):
            v, c = _armi.ctypes.c_double(), _armi.ctypes.c_int64()
            _armi.call("armi_kernel_timing_read", slot, _armi.ctypes.byref(v), _armi.ctypes.byref(c))
            sparse_timing[key] = (v.value, c.value)
    rr_ms = sum(a.elapsed_time(b) for a, b in rr_timing["events"])
    tot_ms, launches = _armi.ctypes.c_double(), _armi.ctypes.c_int64()
    _armi.call("armi_scan_timing_read", _armi.ctypes.byref(tot_ms), _armi.ctypes.byref(launches))
    _armi.call("armi_scan_timing_enable", 0)
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    certified = None
    if full and wl == "dense" and last is not None and last.flags is not None:
        # over every query batch of the run (first-pass certificate; the rest took the second pass)
        if sharded is None:
            fls = []
            for i in range(n_q_batches):
                o = step(i)
                torch.cuda.synchronize()
                fls.append(o.flags.clone())
            fl = torch.cat(fls)
        else:
            fl = last.flags
        certified = float((fl == 1).float().mean().item())

    # p50 latency of one step (batch of 64 per GPU) and of a single query
    lat, lat1 = [], []
    latency_iters = args.latency_iters if full else 0
    for i in range(latency_iters):
        barrier()
        t1 = time.perf_counter()
        step(i)
        barrier()
        lat.append(time.perf_counter() - t1)
    for i in range(latency_iters):
        barrier()
        t1 = time.perf_counter()
        step(i, queries[i % n_q_batches][:1])
        barrier()
        lat1.append(time.perf_counter() - t1)

    if rank != 0:
        if distributed:
            dist.barrier()
            dist.destroy_process_group()
        return

    total_queries = world * batch * args.steps
    scan_avg_ms = tot_ms.value / launches.value if launches.value else float("nan")
    shard_rows = hi - lo
    nq_scan = world * batch  # queries each rank's scan processes per step (all-gathered)
    form = index.scan_form(nq_scan, pre_k)  # which scan armi_dense_topk ran (include/armi.h)
    if form == _armi.SCAN_INT8_FILTER:
        # int8 filter image (1 B / component) + a32, e32 (8 B / row) + the fp16 queries
        alg_bytes = shard_rows * dim + shard_rows * 8 + nq_scan * dim * 2
        nt = "true" if index.scan_nontemporal(nq_scan, pre_k) else "false"
        scan_kernel = f"dense_scan_i8_kernel<{dim}, false, {nt}>"
    elif form == _armi.SCAN_TILED_INT8:
        # int8 image + a32, e32 per row; the call's int8 queries (1 B / component)
        alg_bytes = shard_rows * dim + shard_rows * 8 + nq_scan * dim
        scan_kernel = f"dense_gemm_scan_w4_kernel<{dim}, 0, true>"
    else:
        alg_bytes = shard_rows * dim * 2 + shard_rows * 4 + nq_scan * dim * 2
        scan_kernel = (f"dense_scan_kernel<{dim}>" if form == _armi.SCAN_FP16
                       else f"dense_gemm_scan_w4_kernel<{dim}, 0, false>")
    alg_flops = 2.0 * shard_rows * dim * nq_scan
    # the scan's bound: HBM while the batch is small (arithmetic intensity ~ queries/pass flop/B),
    # the MFMA (fp16, or int8 for the int8 tiled form: 2x the fp16 rate) once the all-gathered
    # batch of a multi-GPU step passes the ridge
    mfma_dtype = "i8" if form == _armi.SCAN_TILED_INT8 else "fp16"
    mfma_bound = alg_flops / (MFMA_PEAK_TFLOPS[mfma_dtype] * 1e12) > alg_bytes / (HBM_PEAK_GBS * 1e9)
    achieved = alg_bytes / (scan_avg_ms * 1e-3) / 1e9
    traffic, traffic_src = (read_traffic(traffic_key(form, shard_rows, dim, nq_scan, args.corpus),
                                         scan_kernel) if world == 1 else (None, None))
    result = {
        "metric": METRIC,
        "value": total_queries / elapsed,
        "unit": "queries/sec",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f16",
        "data": ("synthetic: N(0,1) rows and queries L2-normalised then cast to fp16 (SURVEY.md "
                 "§8(d)), resident in HBM" if args.corpus == "random" else
                 "synthetic clustered lecture corpus (synthetic.make_clustered_rows: mean "
                 "direction, topics, overlapping-chunk near-duplicate runs, re-uploads) and "
                 "queries near random chunks, fp16, resident in HBM"),
        "config": {
            "workload": {
                "dense": (f"dense cosine top-{k} over {n} x {dim} fp16 chunks sharded by ordinal over "
                          f"{world} GPU(s), {batch} queries per GPU per step (RCCL all-gather of "
                          f"queries and per-shard top-{k} when N>1)"),
                "hybrid": (f"hybrid top-{search_k}: dense cosine + sparse lexical prefetch {pre_k} "
                           f"each, RRF (1/(2+pos)), {n} chunks, {batch} queries per GPU per step "
                           f"(configs[2]'s retrieval, no rerank)"),
                "hybrid_rerank": (f"hybrid top-{search_k} (prefetch {pre_k}+{pre_k}, RRF) -> "
                                  f"cross-encoder (XLM-R base, 12 layers, L=256, "
                                  f"{args.rerank_dtype} GEMMs) -> top-{k}, {n} chunks, {batch} "
                                  f"queries per GPU per step"),
            }[wl],
            "n_chunks": n, "dim": dim, "batch_per_gpu": batch, "top_k": k, "corpus": args.corpus,
            "parallelism": f"corpus-shard{world}" + ("" if backend == "nccl" or world == 1
                                                      else f" ({backend} rehearsal, shared GPUs)"),
        },
        "p50_ms": statistics.median(lat) * 1e3 if lat else None,
        "p50_single_query_ms": statistics.median(lat1) * 1e3 if lat1 else None,
        "certified_frac": certified,
        "roofline": ({
            "bound": "hbm",
            "kernel": scan_kernel,
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic,
            "traffic_source": traffic_src,
            "traffic_over_algorithmic": traffic / alg_bytes if traffic else None,
            "algorithmic_bytes_per_launch": alg_bytes,
            "avg_launch_ms": scan_avg_ms,
            "launches_timed": launches.value,
        } if not mfma_bound else {
            "bound": "mfma",
            "kernel": scan_kernel,
            "achieved": alg_flops / (scan_avg_ms * 1e-3) / 1e12,
            "peak": MFMA_PEAK_TFLOPS[mfma_dtype],
            "unit": "TFLOP/s" if mfma_dtype == "fp16" else "TOPS (int8)",
            "frac": alg_flops / (scan_avg_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[mfma_dtype],
            "frac_of_measured_ceiling": (alg_flops / (scan_avg_ms * 1e-3) / 1e12
                                         / MFMA_PRACTICAL_TFLOPS["fp16"]
                                         if mfma_dtype == "fp16" else None),
            "traffic": None,
            "algorithmic_flops_per_launch": alg_flops,
            "algorithmic_bytes_per_launch": alg_bytes,
            "hbm_gbs_achieved": achieved,
            "avg_launch_ms": scan_avg_ms,
            "launches_timed": launches.value,
        }),
    }
    if not launches.value:
        # no timed launch of the scan (fewer steps than the timing period, or graph replays in a
        # plain hybrid run): no roofline rather than one of NaNs
        result["roofline"] = None
    if reranker is not None and rr_timing["events"]:
        # configs[2]: the cross-encoder is the dominant (MFMA-bound) stage; the scan roofline
        # moves to roofline_scan
        rr_tflops = rr_timing["flops"] / (rr_ms * 1e-3) / 1e12
        peak = MFMA_PEAK_TFLOPS[args.rerank_dtype]
        result["roofline_scan"] = result["roofline"]
        result["roofline"] = {
            "bound": "mfma",
            "kernel": f"cross-encoder forward ({args.rerank_dtype} GEMMs, fused attention)",
            "achieved": rr_tflops,
            "peak": peak,
            "unit": "TFLOP/s",
            "frac": rr_tflops / peak,
            "frac_of_measured_ceiling": (rr_tflops / MFMA_PRACTICAL_TFLOPS[args.rerank_dtype]
                                         if args.rerank_dtype in MFMA_PRACTICAL_TFLOPS else None),
            "traffic": None,
            "algorithmic_flops_per_step": rr_timing["flops"] / max(len(rr_timing["events"]), 1),
            "avg_forward_ms": rr_ms / max(len(rr_timing["events"]), 1),
            "forwards_timed": len(rr_timing["events"]),
        }
        result["rerank_share_of_step"] = (rr_ms * 1e-3) / elapsed
    if full and sindex is not None and world == 1:
        # sparse roofline of the dominant sparse kernel. With the MFMA filter (every query of a
        # pass answered by it: ARMI_FLAG_FILTERED) that is sparse_filter_scan_kernel, whose
        # algorithmic bytes per 64-query pass are the u8 levels of the pass's dense-column terms
        # (1 B per row and term, df >= rows/8) + 8 B (row int32 + value fp32) per posting of its
        # other terms; the exact scan reads 4 B per row of a dense-column term instead.
        sp_ms, sp_n = sparse_timing.get("scan_alone", (0.0, 0))
        st_ms, st_n = sparse_timing.get("stage_alone", (0.0, 0))
        fl = torch.cat([sindex.topk(*qs, pre_k, workspace=sws).flags for qs in q_sparse])
        filtered = float(((fl & _armi.ARMI_FLAG_FILTERED) != 0).float().mean())
        post = torch.bincount(csr[1].long(), minlength=VOCAB)
        # the filter's u8 columns: terms in >= 1/32 of the rows; the exact scan's fp32 columns:
        # terms in >= 1/8
        col_bytes, col_frac = (1, 32) if filtered == 1.0 else (4, 8)

        def term_bytes(df: torch.Tensor) -> float:
            dense = df * col_frac >= n
            return float(torch.where(dense, torch.full_like(df, col_bytes * n), 8 * df).sum())

        pass_bytes = [term_bytes(post[torch.unique(qs[1].long())]) for qs in q_sparse]
        alg = sum(pass_bytes[i % n_q_batches] for i in range(args.steps)) / max(args.steps, 1)
        sp_kernel = "sparse_filter_scan_kernel" if filtered == 1.0 else "sparse_scan_kernel<false>"
        def avg_ms(key):
            v, c = sparse_timing.get(key, (0.0, 0))
            return v / c if c else None

        if sp_n:
            sp_avg = sp_ms / sp_n
            sp_traffic, sp_src = read_traffic(f"sparse_scan_{args.corpus}_n{n}_q{batch}", sp_kernel)
            result["roofline_sparse"] = {
                "bound": "hbm", "kernel": sp_kernel, "achieved": alg / (sp_avg * 1e-3) / 1e9,
                "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": alg / (sp_avg * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": sp_traffic,
                "traffic_source": sp_src,
                "traffic_over_algorithmic": sp_traffic / alg if sp_traffic else None,
                "algorithmic_bytes_per_launch": alg, "avg_launch_ms": sp_avg,
                "launches_timed": sp_n,
                "avg_launch_ms_in_step": avg_ms("scan_in_step"),
                "note": ("algorithmic bytes = sum over the distinct terms of the 64-query pass of "
                         f"{col_bytes} B per row for a column term (df >= rows/{col_frac}) and 8 B "
                         "per posting of the others; avg_launch_ms = the kernel alone on the GPU "
                         "(the step's sparse calls re-run by themselves after the timed region), "
                         "avg_launch_ms_in_step = inside eager hybrid steps, sharing the GPU with "
                         "the dense scan on the other stream")}
        if st_n:
            result["sparse_stage"] = {
                "avg_call_ms": st_ms / st_n, "calls_timed": st_n,
                "avg_call_ms_in_step": avg_ms("stage_in_step"),
                "filtered_frac": filtered,
                "note": "one armi_sparse_topk call of 64 queries (pass_terms, filter prep / scan / "
                        "merge, the exact scan's early exit and its merge / collect launches), "
                        "HIP events around the call on its stream; avg_call_ms alone on the GPU, "
                        "avg_call_ms_in_step concurrent with the dense chain"}
    if scan_timing_note:
        result["scan_timing"] = scan_timing_note
    result["cpu_baseline"] = None
    if full and world == 1 and not args.no_cpu_baseline:
        ref = CpuReference(rows, csr)
        qn = queries.reshape(-1, dim).float().cpu().numpy()
        q_csr = None
        if csr is not None:
            q_csr = []
            for qp, qi, qv in q_sparse:
                qp, qi, qv = qp.cpu().numpy(), qi.cpu().numpy(), qv.cpu().numpy()
                q_csr += [(qi[qp[b]:qp[b + 1]], qv[qp[b]:qp[b + 1]]) for b in range(qp.size - 1)]
        pairs = None
        if hf_reranker is not None:
            nr = 8
            hits = [ref.hybrid_one(qn[i], q_csr[i][0], q_csr[i][1], search_k) for i in range(nr)]
            ords = torch.tensor([[h[0] for h in hs] for hs in hits], dtype=torch.int64)
            qt = q_tokens[0][:nr].cpu().to(torch.int64)
            kc = ords.shape[1]
            bos = torch.zeros((nr, kc, 1), dtype=torch.int64)
            eos = torch.full((nr, kc, 1), 2, dtype=torch.int64)
            pairs = (hf_reranker, torch.cat([bos, qt[:, None, :].expand(nr, kc, qt.shape[1]), eos, eos,
                                             doc_tokens(ords, 236).to(torch.int64), eos], dim=2))
        result["cpu_baseline"] = cpu_baseline(wl, ref, qn, q_csr, k, search_k, pairs,
                                              budget_s=args.cpu_budget)
        del ref
    if full and wl == "dense" and world == 1 and not args.no_extras and args.corpus == "random":
        result.update(secondary_configs(args))
    print(json.dumps(result), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


def secondary_configs(args) -> dict:
    """BASELINE configs[1] and configs[2], north_star's 10k / 10M ends of the size sweep,
    configs[2]'s retrieval alone ("hybrid"), the single-stream AudioRAG.query() pipeline and
    configs[3]'s per-rank call, measured beside the headline (the driver runs only the default
    bench line): each is a child bench.py run on the same GPU, its JSON line attached under its
    key (value, ms_per_step, p50, rooflines)."""
    import subprocess

    # configs1 / configs2 carry their own cpu_baseline (dense at 100k; the reference's hybrid +
    # cross-encoder path at 1M), each leg bounded by a shorter budget
    cpu = ["--cpu-budget", "10"]
    runs = {
        "configs1": ["--chunks", "100000", "--steps", "200", "--warmup", "10",
                     "--latency-iters", "20", *cpu],
        "configs2": ["--workload", "hybrid_rerank", "--chunks", str(args.chunks), "--steps", "10",
                     "--warmup", "2", "--latency-iters", "3", *cpu],
        # north_star's size sweep (10k / 100k / 1M / 10M chunks): the two ends besides configs1
        # and the headline
        "chunks_10k": ["--chunks", "10000", "--steps", "200", "--warmup", "10",
                       "--latency-iters", "10"],
        "chunks_10M": ["--chunks", "10000000", "--steps", "20", "--warmup", "3",
                       "--latency-iters", "3"],
        # configs[2]'s retrieval alone (dense + sparse prefetch 40 each, RRF 20; no rerank), with
        # the sparse stage's roofline and the reference's hybrid CPU path beside it
        "hybrid": ["--workload", "hybrid", "--chunks", str(args.chunks), "--steps", "100",
                   "--warmup", "10", "--latency-iters", "10", *cpu],
        # AudioRAG.query() one query at a time over the 1M-chunk hybrid store, per-stage p50s
        "pipeline": ["--workload", "pipeline", "--chunks", str(args.chunks), "--queries", "100"],
        # configs[3]'s per-rank call on one GPU: 10M chunks / 8 ranks = 1.25M rows x the 8 x 64
        # all-gathered queries, top-5 (collectives excluded: per-rank work, not a scaling number)
        "configs3_rank": ["--chunks", "1250000", "--batch", "512", "--steps", "20", "--warmup",
                          "3", "--latency-iters", "3"],
    }
    out = {}
    for key, extra in runs.items():
        cmd = [sys.executable, str(ROOT / "bench.py"), "--full", "--no-extras", *extra]
        if key not in ("configs1", "configs2", "hybrid"):
            cmd.append("--no-cpu-baseline")
        try:
            t_child = time.perf_counter()
            # the child's stderr passes through (progress on long runs); stdout is its JSON line
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True,
                                 timeout=480 if key == "pipeline" else 300)
            print(f"[bench] {key}: rc {res.returncode} in {time.perf_counter() - t_child:.0f} s",
                  file=sys.stderr, flush=True)
            line = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
            d = json.loads(line) if res.returncode == 0 and line.startswith("{") else None
        except (subprocess.TimeoutExpired, json.JSONDecodeError):
            d = None
        if d is None:
            out[key] = {"error": "child bench run failed", "cmd": " ".join(cmd[1:])}
            continue
        keep = ("value", "unit", "ms_per_step", "steps", "p50_ms", "p50_single_query_ms",
                "p95_ms", "p99_ms", "stage_p50_ms", "reference_published_p50_ms",
                "certified_frac", "config", "roofline", "roofline_scan", "roofline_sparse",
                "sparse_stage", "rerank_share_of_step", "dtype", "cpu_baseline")
        out[key] = {kk: d[kk] for kk in keep if kk in d}
        if key in ("configs1", "configs2"):
            out[key]["baseline_config"] = {"configs1": 1, "configs2": 2}[key]
        if key == "configs3_rank":
            out[key]["baseline_config"] = 3
            out[key]["note"] = ("per-rank work of configs[3] measured on one GPU: one rank's "
                                "1.25M-row shard of 10M chunks and the 8 x 64 queries an 8-GPU "
                                "step all-gathers, top-5; collectives excluded, so this is not a "
                                "scaling measurement (the driver's SCALE run is)")
    return out


WORDS = ("gradient descent learning rate loss function model training data neural network layer "
         "weights bias optimizer batch epoch regression classification feature vector matrix "
         "probability distribution bayes kernel margin support vector tree boosting variance "
         "lecture professor example equation derivative convex objective parameter sample").split()


def pipeline_main(args) -> None:
    """The reference's query path one query at a time, as AudioRAG.query() runs it
    (pipeline/query.py:97-215): BGE-M3 query encode (XLM-R large, 24 layers, fp16, HIP-graph
    replay), hybrid search (dense + sparse prefetch 2 x initial_k = 40 each, RRF -> 20) over the
    chunk store, cross-encoder rerank 20 -> 5 (XLM-R base, fp16), RetrievalResult objects; answer
    generation off. Weights are seeded (no checkpoints offline), so only timing is meaningful.
    value = 1 / mean end-to-end latency (one stream); the reference publishes single-GPU
    latencies for the same stages (on a ~100s-of-chunks corpus)."""
    import logging

    from audio_rag_amd.config.schema import AudioRAGConfig
    from audio_rag_amd.embeddings.bge_m3 import BGEM3Embedder
    from audio_rag_amd.pipeline.query import QueryPipeline
    from audio_rag_amd.reranking.bge import BGEReranker
    from audio_rag_amd.retrieval.collection import ChunkCollection
    from audio_rag_amd.retrieval.device import DenseIndex, SparseIndex
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    logging.disable(logging.INFO)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, dim = args.chunks, args.dim
    cfg = AudioRAGConfig()
    cfg.retrieval.search_type = "hybrid"
    rng = np.random.default_rng(11)
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(30, 60)))) for _ in range(4096)]
    payloads = [{"text": texts[i % 4096], "start": float(i), "end": float(i) + 30.0,
                 "speaker": None, "metadata": {}} for i in range(n)]
    rows = make_rows(0, n, dim, dev)
    sindex = SparseIndex(*make_sparse_rows(0, n, dev), vocab=VOCAB)
    ret = MI355XRetriever(cfg.retrieval, dim)
    ret.attach_collection(ChunkCollection.from_indexes(cfg.retrieval.collection_name,
                                                       DenseIndex(rows), payloads, sindex))
    emb = BGEM3Embedder(cfg.embedding, device=dev)
    emb.load()
    rr = BGEReranker(cfg.reranking, device=dev)
    rr.load()
    pipe = QueryPipeline(cfg)
    pipe._embedder, pipe._retriever = emb, ret
    pipe._reranker, pipe._reranker_created = rr, True
    queries = [" ".join(rng.choice(WORDS, size=int(rng.integers(6, 16)))) for _ in range(256)]

    def sync_time(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t

    for q in queries[:16]:  # warm-up: graph capture per length bucket, kernel autotuning
        pipe.query(q, generate_answer=False)
    e2e, t_emb, t_search, t_rerank = [], [], [], []
    for i in range(args.queries):
        q = queries[i % len(queries)]
        res, t = sync_time(lambda: pipe.query(q, generate_answer=False))
        assert res.reranked and len(res.results) == cfg.reranking.top_k
        e2e.append(t)
        e, t = sync_time(lambda: emb.embed_query(q))
        t_emb.append(t)
        hits, t = sync_time(lambda: ret.search(e, top_k=cfg.reranking.initial_k,
                                               search_type="hybrid"))
        t_search.append(t)
        _, t = sync_time(lambda: rr.rerank(q, hits, top_k=cfg.reranking.top_k))
        t_rerank.append(t)
    ms = lambda xs, p: float(np.percentile(np.array(xs) * 1e3, p))
    print(json.dumps({
        "metric": METRIC,
        "value": 1.0 / float(np.mean(e2e)),
        "unit": "queries/sec",
        "n_gpus": 1,
        "steps": args.queries,
        "warmup": 16,
        "ms_per_step": float(np.mean(e2e)) * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f16",
        "data": ("synthetic: seeded BGE-M3 / reranker weights, N(0,1) unit fp16 chunk vectors, "
                 "Zipf sparse vectors, synthetic chunk and query texts"),
        "config": {"workload": (f"QueryPipeline.query() single-stream: BGE-M3 encode -> hybrid "
                                f"search (prefetch 40 + 40, RRF 20) over {n} chunks -> rerank "
                                f"20 -> 5 (fp16), one query at a time"),
                   "n_chunks": n, "dim": dim, "initial_k": cfg.reranking.initial_k,
                   "top_k": cfg.reranking.top_k, "parallelism": "single GPU, batch 1"},
        "p50_ms": ms(e2e, 50), "p95_ms": ms(e2e, 95), "p99_ms": ms(e2e, 99),
        "stage_p50_ms": {"embed": ms(t_emb, 50), "hybrid_search": ms(t_search, 50),
                         "rerank": ms(t_rerank, 50)},
        "reference_published_p50_ms": {"embed": 18, "hybrid_search": 48, "rerank": 38,
                                       "warm_query": 141,
                                       "source": "docs/SALES_TECHNICAL_GUIDE.md:563-565, "
                                                 "README.md:37-38 (single unspecified GPU, "
                                                 "~100s of chunks)"},
        "roofline": None,
        "cpu_baseline": None,
    }), flush=True)


def ingest_main(args) -> None:
    """configs[4] after ASR (faster-whisper is not installed; the reference's ingest stages up to
    the transcript stay out of scope): --ingest-chunks synthetic transcript chunks (40-100 words)
    -> BGEM3Embedder.embed (24-layer XLM-R large fp16, batch_size 32, dense + lexical weights,
    embeddings/bge.py:104-135) -> MI355XRetriever.add (qdrant.py:140-225, reference sparse-drop
    by default) -> the native StreamServer over the new collection under open-loop Poisson load
    at --qps (dense top-k). value = completed streaming queries / s; the embed and index rates
    ride along. Weights are seeded (no checkpoints offline)."""
    import logging

    from audio_rag_amd.config.schema import AudioRAGConfig
    from audio_rag_amd.core.base import AudioChunk
    from audio_rag_amd.embeddings.bge_m3 import BGEM3Embedder
    from audio_rag_amd.retrieval.batcher import StreamServer
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    logging.disable(logging.INFO)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = AudioRAGConfig()
    rng = np.random.default_rng(13)
    n = args.ingest_chunks
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(40, 100)))) for _ in range(n)]
    chunks = [AudioChunk(text=t, start=30.0 * i, end=30.0 * i + 30.0, speaker=f"SPEAKER_{i % 2}",
                         metadata={"lecture": i % 7}) for i, t in enumerate(texts)]
    emb = BGEM3Embedder(cfg.embedding, device=dev)
    emb.load()
    emb.embed(texts[:64])  # warm-up (kernel selection)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    embeddings = emb.embed(texts)
    torch.cuda.synchronize()
    t_embed = time.perf_counter() - t0
    ret = MI355XRetriever(cfg.retrieval, emb.dimension)
    t0 = time.perf_counter()
    ret.add(chunks, embeddings)
    ret._collections[ret._resolve_collection(None)].dense_index  # build the device index
    torch.cuda.synchronize()
    t_index = time.perf_counter() - t0
    q_texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(6, 16)))) for _ in range(256)]
    qd, _ = emb.embed_queries(q_texts)
    qs = qd.cpu().numpy()
    n_q = int(args.qps * args.duration)
    k = cfg.retrieval.top_k
    with StreamServer(ret, top_k=k, max_batch=64, max_wait_ms=args.max_wait_ms) as srv:
        srv.loadgen(qs, min(n_q, 4096), qps=args.qps, seed=6)  # warm-up
        b0, q0 = srv.stats()
        lat, elapsed = srv.loadgen(qs, n_q, qps=args.qps, seed=7)
        b1, q1 = srv.stats()
    batches, served = b1 - b0, q1 - q0
    lat_ms = lat * 1e3
    print(json.dumps({
        "metric": METRIC,
        "value": n_q / elapsed,
        "unit": "queries/sec",
        "n_gpus": 1,
        "steps": int(batches),
        "warmup": min(n_q, 4096),
        "ms_per_step": elapsed / max(batches, 1) * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f16",
        "data": ("synthetic transcript chunks (lecture vocabulary), seeded BGE-M3 weights, "
                 "queries embedded by the same model"),
        "config": {"workload": (f"configs[4] after ASR: {n} chunks -> BGE-M3 embed (24 layers "
                                f"fp16, batch {cfg.embedding.batch_size}) -> MI355XRetriever.add "
                                f"-> native StreamServer, open-loop Poisson queries at "
                                f"{args.qps:.0f} q/s for {args.duration:.1f} s, dense top-{k}"),
                   "n_chunks": n, "dim": emb.dimension, "top_k": k, "offered_qps": args.qps,
                   "parallelism": "single GPU"},
        "embed_chunks_per_s": n / t_embed,
        "embed_s": t_embed,
        "index_chunks_per_s": n / t_index,
        "index_s": t_index,
        "p50_ms": float(np.percentile(lat_ms, 50)),
        "p99_ms": float(np.percentile(lat_ms, 99)),
        "mean_batch": served / max(batches, 1),
        "roofline": None,
        "cpu_baseline": None,
    }), flush=True)


def stream_main(args) -> None:
    """configs[4]'s query side on one GPU: single dense queries arrive as an open-loop Poisson
    process at --qps over the 1M-chunk store. Default front end: the native StreamServer
    (libarmi armi_stream_*: coalescing into batches of <= 64, <= --max-wait-ms after a batch's
    first query, up to three batches in flight on the server's stream) driven by libarmi's own
    load generator thread, so no interpreter sits in the request path. --stream-front python:
    the same arrivals from a Python client thread through QueryBatcher (futures +
    list[RetrievalResult] per caller). value = completed queries / s; latency = submit -> result."""
    from audio_rag_amd.config import RetrievalConfig
    from audio_rag_amd.retrieval.batcher import QueryBatcher, StreamServer
    from audio_rag_amd.retrieval.collection import ChunkCollection
    from audio_rag_amd.retrieval.device import DenseIndex
    from audio_rag_amd.retrieval.mi355x import MI355XRetriever

    from audio_rag_amd.retrieval.device import SparseIndex

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n, dim, k = args.chunks, args.dim, args.top_k
    hybrid = args.search_type == "hybrid"
    rows = make_rows(0, n, dim, dev)
    payloads = [{"text": "", "start": 0.0, "end": 0.0, "speaker": None, "metadata": {}}] * n
    ret = MI355XRetriever(RetrievalConfig(top_k=k, search_type=args.search_type), dim)
    sidx = SparseIndex(*make_sparse_rows(0, n, dev), vocab=VOCAB) if hybrid else None
    ret.attach_collection(ChunkCollection.from_indexes("audio_rag", DenseIndex(rows), payloads,
                                                       sidx))
    qs = make_queries(1, 4096, dim, dev, seed=1)[0].cpu().numpy()
    q_csr = tuple(t.cpu().numpy() for t in make_sparse_queries(4096, dev, seed=1000)) if hybrid else None
    n_q = int(args.qps * args.duration)
    if args.stream_front == "native":
        with StreamServer(ret, max_batch=args.max_batch, max_wait_ms=args.max_wait_ms,
                          search_type=args.search_type) as srv:
            srv.loadgen(qs, 4096, qps=args.qps, seed=6, sparse_csr=q_csr)  # warm-up
            b0, q0 = srv.stats()
            lat, elapsed = srv.loadgen(qs, n_q, qps=args.qps, seed=7, sparse_csr=q_csr)
            b1, q1 = srv.stats()
        batches, served = b1 - b0, q1 - q0
        value = n_q / elapsed
        front = "native StreamServer + native open-loop load generator"
    else:
        # the client thread and the batcher thread share one interpreter: hand the GIL over at
        # 0.2 ms instead of the 5 ms default, or a batch waits for the client's time slice
        sys.setswitchinterval(2e-4)
        rng = np.random.default_rng(7)
        lat_l, done = [], []
        lock = __import__("threading").Lock()

        def on_done(t_sub):
            def cb(f):
                t = time.perf_counter()
                f.result()
                with lock:
                    lat_l.append(t - t_sub)
                    done.append(t)
            return cb

        sp = (lambda i: (q_csr[1][q_csr[0][i]:q_csr[0][i + 1]], q_csr[2][q_csr[0][i]:q_csr[0][i + 1]])
              ) if hybrid else (lambda i: None)
        with QueryBatcher(ret, max_batch=64, max_wait_ms=args.max_wait_ms) as qb:
            for i in range(256):  # warm-up
                qb.submit_arrays(qs[i % 4096], sp(i % 4096)).result()
            gaps = rng.exponential(1.0 / args.qps, size=n_q)
            t0 = time.perf_counter()
            t_next = t0
            futs = []
            for i in range(n_q):
                t_next += gaps[i]
                delay = t_next - time.perf_counter()
                if delay > 0:
                    time.sleep(delay)  # releases the GIL to the batcher thread (never spin here)
                f = qb.submit_arrays(qs[i % 4096], sp(i % 4096))
                f.add_done_callback(on_done(time.perf_counter()))
                futs.append(f)
            for f in futs:
                f.result()
            batches, served = qb.batches - 0, qb.queries
        lat = np.array(lat_l)
        elapsed = max(done) - t0
        value = len(done) / elapsed
        front = "Python client thread + QueryBatcher (futures, list[RetrievalResult])"
    lat_ms = np.asarray(lat) * 1e3
    print(json.dumps({
        "metric": METRIC,
        "value": value,
        "unit": "queries/sec",
        "n_gpus": 1,
        "steps": int(batches),
        "warmup": 4096 if args.stream_front == "native" else 256,
        "ms_per_step": elapsed / max(batches, 1) * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f16",
        "data": "synthetic: N(0,1) rows and queries L2-normalised then cast to fp16, resident in HBM",
        "config": {"workload": (f"streaming {args.search_type} top-{k}"
                                + (f" (prefetch {2 * k} + {2 * k}, RRF)" if hybrid else "")
                                + ": open-loop Poisson arrivals at "
                                f"{args.qps:.0f} q/s for {args.duration:.1f} s, {front}, batches "
                                f"<= {args.max_batch} / <= {args.max_wait_ms} ms -> exact cosine "
                                f"top-{k} over "
                                f"{n} x {dim} fp16 chunks"
                                + (" + Zipf sparse vectors" if hybrid else "")),
                   "n_chunks": n, "dim": dim, "top_k": k, "offered_qps": args.qps,
                   "front_end": args.stream_front, "search_type": args.search_type,
                   "parallelism": "single GPU, batching server"},
        "p50_ms": float(np.percentile(lat_ms, 50)),
        "p99_ms": float(np.percentile(lat_ms, 99)),
        "mean_batch": served / max(batches, 1),
        "roofline": None,
        "cpu_baseline": None,
    }), flush=True)


if __name__ == "__main__":
    main()
