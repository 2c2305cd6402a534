#!/usr/bin/env python3
"""Sweep of tuning knob walk_table_early_wgs (walk_plan.h: the level-table GEMM in two parts) on bench.py's main workload in ONE process:
the corpus and the graph are built once, every setting is measured like bench.py's timed region (5 warm-up + 20 timed steps of 32 768
queries at ef 112, two launches in flight), the settings interleaved over several rounds.  One JSON line per measurement.
usage: table_early_wgs_sweep.py [--values 0,16,24,32,48,64,96] [--rounds 2] [--out profiles/NAME.jsonl]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
import cosdata_amd as ca
from cosdata_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--values", default="0,16,24,32,48,64,96")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--out", default="table_early_wgs_sweep.jsonl")
a = ap.parse_args()
args = argparse.Namespace(top_k=10, batch=256, coalesce=128, inflight=0, recall_queries=8192, steps=20, warmup=5)
env = bench.Env(args)
t0 = time.time()
wl = bench.DenseWorkload(env, bench.MAIN_WORKLOAD, append_rows=100_000)
hp = ca.HNSWHyperParams(num_layers=9, ef_construction=wl.ef_construction, ef_search=112, level_0_neighbors_count=bench.MAIN_M0, neighbors_count=bench.MAIN_M)
ix = ca.HNSWIndex(wl.d, hp, ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), wl.values_range, shortlist_size=64, device=0, id_base=0, seed=42,
                  visited_mode=ca.VISITED_REF)
ix.upload_vectors_device(wl.X.data_ptr(), wl.n, keepalive=wl.X)
ix.build(wl.build_batch)
print(f"corpus + graph in {time.time() - t0:.1f} s", flush=True)
B, k, S = wl.B, wl.k, wl.S

def step(i):
    s = i % S
    q = wl.Q[(i % wl.n_qsets) * B:(i % wl.n_qsets + 1) * B]
    ix.batch_search_device(q.data_ptr(), B, k, wl.o_ids[s].data_ptr(), wl.o_sc[s].data_ptr(), wl.o_cnt[s].data_ptr(), wl.o_st[s].data_ptr(), wl.streams[s].cuda_stream)

def run(n_warm=5, n_launch=20):
    for i in range(n_warm):
        step(i)
    env.sync_all()
    ix.enable_timing(True)
    t = time.perf_counter()
    for i in range(n_warm, n_warm + n_launch):
        step(i)
    env.sync_all()
    el = time.perf_counter() - t
    sp = [ix.last_walk_split(wl.streams[s].cuda_stream) for s in range(S)]
    ix.enable_timing(False)
    m = lambda f: float(np.mean([f(x) for x in sp]))
    ids = wl.o_ids[(n_warm + n_launch - 1) % S].cpu().numpy().copy()
    global planned
    planned = int(sp[0].table_early_wgs)
    return {"ms_per_step": el / n_launch * 1e3, "table_ms": m(lambda x: x.table_ms), "upper_ms": m(lambda x: x.upper_ms), "sort_ms": m(lambda x: x.sort_ms),
            "lower_ms": m(lambda x: x.lower_ms), "table_cols": int(sp[0].table_cols)}, ids

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
run()  # first touch of everything
ref_ids = None
with open(a.out, "a") as fh:
    for r in range(a.rounds):
        for v in [int(x) for x in a.values.split(",")]:
            with _lib.tuning(walk_table_early_wgs=v):
                rec, ids = run()
            if ref_ids is None:
                ref_ids = ids
            rec.update({"walk_table_early_wgs": v, "planned_early_wgs": planned, "round": r, "same_ids_as_first": bool(np.array_equal(ids, ref_ids)), "failed": int((wl.o_st != 0).sum().item())})
            line = json.dumps(rec)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
