"""All-label windowed marginals against L single-label passes, and the typed cluster CRF end to end.

    python tools/bench_typed.py [--items 200000] [--window 20] [--labels 3,8,16,32] [--e2e-genes 2000000] [--out FILE]

Per label count, one JSON line: a plan on device-resident arrays of a synthetic set (the contig-length law and the
attribute count of tools/bench_train_labels.py, weights N(0, 0.5)), `run_windowed_all` with a background label against
`run_windowed` once per label on the same plan and arrays.  Both are timed with HIP events on the null stream
(`time_windowed_all` / `time_windowed`: warm-up launches, then the mean of `--iters` back-to-back launches); a sample of
the single-label path is the sum of its L per-label means.  The two alternate sample by sample, `--samples` times; median,
minimum and maximum are reported, and `ahead` says whether the slowest all-label sample beat the fastest L-pass sample.

Then one line for `TypedClusterCRF.predict_clusters`: a model fitted on the planted set of tests/typed_planted.py, its
4 fresh contigs, and the same contigs repeated under new names up to `--e2e-genes` genes; the host's clock around the
call, and around the device pass alone on the packed arrays."""
import argparse
import itertools
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gecco_amd import _native, model as gmodel, packing, synth, typed  # noqa: E402


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def run_labels(L, args):
    rng = np.random.default_rng(synth.SEED + L)
    W, A = args.window, args.attrs
    lengths = np.maximum(synth.contig_lengths(rng, max(1, args.items // 200), total_genes=args.items), W)
    cptr, gptr, attr = synth.synth_contigs(rng, lengths, A)
    n = int(cptr[-1])
    m = _native.Model.from_tables(rng.normal(0, 0.5, size=(A, L)), rng.normal(0, 0.5, size=(L, L)))
    plan = _native.Plan(m, cptr, W, 1, True, device=0)
    dev = torch.device("cuda:0")
    d_gp, d_at = torch.from_numpy(gptr).to(dev), torch.from_numpy(attr).to(dev)
    p_all = torch.zeros(n, L, dtype=torch.float64, device=dev)
    p_any = torch.zeros(n, dtype=torch.float64, device=dev)
    p_one = torch.zeros(n, dtype=torch.float64, device=dev)
    gp, at = d_gp.data_ptr(), d_at.data_ptr()
    all_ms, single_ms = [], []
    for _ in range(args.samples):
        all_ms.append(plan.time_windowed_all(gp, at, p_all.data_ptr(), p_any.data_ptr(), background=0, warmup=args.warmup,
                                             iters=args.iters))
        single_ms.append(sum(plan.time_windowed(gp, at, p_one.data_ptr(), label=l, warmup=args.warmup, iters=args.iters)
                             for l in range(L)))
    torch.cuda.synchronize()
    # the two paths agree (2e-12: each is within 1e-12 of the oracle)
    plan.run_windowed(gp, at, p_one.data_ptr(), label=L - 1)
    torch.cuda.synchronize()
    diff = float((p_all[:, L - 1] - p_one).abs().max())
    return {"tool": "bench_typed", "labels": L, "window": W, "items": n, "contigs": len(lengths), "attrs": A,
            "all_kernel": plan.all_kernel_name, "single_kernel": plan.kernel_name, "all_ms": stats(all_ms),
            "single_x_L_ms": stats(single_ms), "ratio_single_over_all": float(np.median(single_ms) / np.median(all_ms)),
            "ahead": bool(max(all_ms) < min(single_ms)), "samples": args.samples, "iters": args.iters,
            "all_genes_per_s": n / (np.median(all_ms) * 1e-3), "max_abs_diff_last_label": diff}


def repeated(genes, total):
    """The genes of `genes` (whole contigs) under new sequence names until `total` genes are reached."""
    contigs = [list(g) for _, g in itertools.groupby(genes, key=lambda g: g.source.id)]
    out, r = [], 0
    while len(out) < total:
        for contig in contigs:
            src = gmodel.Source(f"{contig[0].source.id}_r{r:05d}")
            out.extend(gmodel.Gene(src, g.start, g.end, g.strand, gmodel.Protein(f"{g.protein.id}_r{r}", None, g.protein.domains))
                       for g in contig)
        r += 1
    return out


def clock(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, stats(times)


def run_end_to_end(args):
    from tests.typed_planted import C, W, cluster_table as _cluster_table, planted_set as _set

    train_genes, rows = _set(11, 12, "train", composite=True)
    fresh, _ = _set(12, 4, "fresh", composite=False)
    random.seed(42)
    crf = typed.TypedClusterCRF(W, 1, c1=C, c2=C).fit(train_genes, _cluster_table(rows))
    out = {"tool": "bench_typed", "end_to_end": "TypedClusterCRF.predict_clusters", "labels": len(crf.classes_), "window": W}
    for name, genes, repeats in (("four_contigs", fresh, 7), ("large", repeated(fresh, args.e2e_genes), 3)):
        if not genes:
            continue
        crf.predict_clusters(genes)  # (warm-up: library, plan tables, allocations)
        clusters, total = clock(lambda: crf.predict_clusters(genes), repeats)
        srt = sorted(genes, key=lambda g: (g.source.id, g.start))
        contigs = [list(g) for _, g in itertools.groupby(srt, key=lambda g: g.source.id)]
        batch = packing.pack_contigs(contigs, crf._attr_index, "protein")
        ip, ap = batch.item_ptr.astype(np.int32), batch.attr_ptr.astype(np.int32)
        _, device = clock(lambda: crf._model.windowed_marginals_all(ip, ap, batch.attr_id, W, 1, background=0), repeats)
        out[name] = {"genes": len(genes), "contigs": len(contigs), "clusters": len(clusters), "predict_clusters_s": total,
                     "device_pass_with_copies_s": device, "host_share": 1.0 - device["median"] / total["median"]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--items", type=int, default=200_000)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--labels", default="3,8,16,32")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--e2e-genes", type=int, default=2_000_000, help="genes of the large end-to-end set (0: skip it)")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")

    for x in args.labels.split(","):
        if x:
            emit(run_labels(int(x), args))
    if not args.no_e2e:
        emit(run_end_to_end(args))


if __name__ == "__main__":
    main()
