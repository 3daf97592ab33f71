"""Constrained-inference benchmark: whole-sequence marginals and Viterbi under allowed-label masks against the same calls
without masks, on the equal set of tools/bench_train_sequences.py (1 000 sequences of 200 items).

    python tools/bench_constrained.py [--sequences 1000] [--length 200] [--labels 2,8,32] [--out FILE]

Per label count one JSON line.  Both sides are one-shot calls of ``_native.Model`` with every attribute value 1.0, so both
take the any-L kernels at every label count (2 included) and differ in the masked state-score kernel alone: ``masked`` passes
random non-empty label sets (every label in with probability 1/2), ``full`` passes masks that allow every label (the masked
kernel, the unmasked results), ``unmasked`` passes none.  The three are timed in turn, call by call, so that drift of the
machine reaches all alike; times are taken as in tools/bench_train_sequences.py (host clock and two HIP events on the null
stream around the synchronous call, which holds the plan, the upload of the batch, the launches and the download)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import _native, synth  # noqa: E402


def random_masks(rng, n, L):
    bits = rng.random((n, L)) < 0.5
    for i in np.flatnonzero(~bits.any(axis=1)):
        bits[i, int(rng.integers(0, L))] = True
    return (bits.astype(np.uint64) << np.arange(L, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)


def timed_in_turn(fns, warmup, evals):
    """name -> median, minimum and maximum in microseconds (host clock, HIP events) of `evals` calls of every function, the
    functions called in turn."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    host, device = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(evals):
        for name, fn in fns.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            stop.record()
            stop.synchronize()
            host[name].append((t1 - t0) * 1e6)
            device[name].append(start.elapsed_time(stop) * 1e3)
    stats = lambda v: [float(np.median(v)), float(min(v)), float(max(v))]
    return {k: {"host_us": stats(host[k]), "hip_event_us": stats(device[k])} for k in fns}


def run(L, args):
    rng = np.random.default_rng(synth.SEED + L)
    A = args.attrs
    model = _native.Model.from_tables(rng.normal(0, 0.5, size=(A, L)), rng.normal(0, 0.5, size=(L, L)))
    seq_ptr, item_ptr, attr = synth.synth_contigs(rng, [args.length] * args.sequences, A)
    n = int(seq_ptr[-1])
    ones = np.ones(len(attr))
    masks = {"masked": random_masks(rng, n, L), "full": np.full(n, (1 << L) - 1, dtype=np.uint32), "unmasked": None}
    out = {"tool": "bench_constrained", "labels": L, "attrs": A, "items": n, "sequences": args.sequences, "entries": int(len(attr)),
           "warmup": args.warmup, "evals_timed": args.evals}
    for entry, call in (("marginals_full", model.marginals_full), ("viterbi", model.viterbi)):
        fns = {name: (lambda m=m: call(seq_ptr, item_ptr, attr, device=args.device, values=ones, allowed=m)) for name, m in masks.items()}
        same = all(a.tobytes() == b.tobytes() for a, b in zip(fns["full"](), fns["unmasked"]()))
        rec = timed_in_turn(fns, args.warmup, args.evals)
        rec["full_masks_give_the_unmasked_bytes"] = bool(same)
        rec["masked_over_unmasked"] = rec["masked"]["hip_event_us"][0] / rec["unmasked"]["hip_event_us"][0]
        rec["full_over_unmasked"] = rec["full"]["hip_event_us"][0] / rec["unmasked"]["hip_event_us"][0]
        out[entry] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("bench_constrained needs a HIP device")
    lines = [json.dumps(run(int(L), args)) for L in args.labels.split(",")]
    for line in lines:
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
