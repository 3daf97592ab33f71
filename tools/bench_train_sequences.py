"""Whole-sequence training benchmark (a sibling of tools/bench_train_labels.py): one objective + gradient evaluation of
gecco_crf_trainer_sequences_eval per label count, on equal sequences and on one lone long sequence, beside the windowed
evaluation (gecco_crf_trainer_general_eval, W = 20, step 1) of the same items.

    python tools/bench_train_sequences.py [--sequences 1000] [--length 200] [--lone 20000] [--labels 2,8,32] [--out FILE]

Per label count it prints one JSON line.  Every time is taken twice around the synchronous call: by the host's clock, as
in tools/bench_train_labels.py, and by two HIP events recorded on the null stream before and after the call.  The library
runs on a stream of its own and ends every evaluation in a stream synchronise, so both clocks hold the same work: the
gather of the weights into the dense tables, the upload, the launches (five for whole sequences, six for windows), the
download and the scatter into g.  The kernels' own times come from a kernel trace of this tool in a run of its own
(``rocprofv3 --kernel-trace --stats -- python tools/bench_train_sequences.py ...``)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import _native, synth  # noqa: E402


def labelled_set(rng, lengths, A, L, stay=0.95):
    """Sequences of the given lengths with synth's attributes, labels from a Markov chain over L labels, the attributes
    moved by label so that the labels can be learned (as tools/bench_train_labels.py)."""
    seq_ptr, item_ptr, attr = synth.synth_contigs(rng, lengths, A)
    n = int(seq_ptr[-1])
    jump = rng.random(n) >= stay
    jump[0] = True
    drawn = rng.integers(0, L, size=n)
    labels = drawn[np.maximum.accumulate(np.where(jump, np.arange(n), 0))].astype(np.int32)
    owner = np.repeat(np.arange(n), np.diff(item_ptr))
    attr = ((attr + labels[owner].astype(np.int64) * A // L) % A).astype(np.int32)
    return seq_ptr, item_ptr, attr, labels


def timed(fn, warmup, evals):
    """Median, minimum and maximum of `evals` calls in microseconds, by the host's clock and by HIP events."""
    for _ in range(warmup):
        fn()
    host, device = [], []
    for _ in range(evals):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        stop.record()
        stop.synchronize()
        host.append((t1 - t0) * 1e6)
        device.append(start.elapsed_time(stop) * 1e3)
    return {"host_us": [float(np.median(host)), float(min(host)), float(max(host))],
            "hip_event_us": [float(np.median(device)), float(min(device)), float(max(device))], "evals_timed": evals}


def run(L, args):
    rng = np.random.default_rng(synth.SEED + L)
    A = args.attrs
    K = A * L + L * L
    sfid, tfid = np.arange(A * L, dtype=np.int32), A * L + np.arange(L * L, dtype=np.int32)
    w = rng.normal(0, 0.5, size=K)
    out = {"tool": "bench_train_sequences", "labels": L, "attrs": A, "features": K}
    for name, lengths in (("equal", [args.length] * args.sequences), ("lone", [args.lone])):
        seq_ptr, item_ptr, attr_id, labels = labelled_set(rng, lengths, A, L)
        whole = _native.TrainerSequences([(seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K)])
        windowed = _native.TrainerGeneral([(seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K, args.window, 1)])
        f, _ = whole.eval([w])
        rec = {"sequences": len(lengths), "items": int(seq_ptr[-1]), "nnz": int(item_ptr[-1]), "f": float(f[0]),
               "whole": timed(lambda: whole.eval([w]), args.warmup, args.evals), "scratch_bytes": whole.scratch_bytes(0),
               "windowed": dict(timed(lambda: windowed.eval([w]), args.warmup, args.evals), window=args.window,
                                windows=windowed.num_windows(0), scratch_bytes=windowed.scratch_bytes(0))}
        rec["ns_per_item"] = rec["whole"]["hip_event_us"][0] * 1e3 / rec["items"]
        rec["whole_over_windowed"] = rec["whole"]["hip_event_us"][0] / rec["windowed"]["hip_event_us"][0]
        out[name] = rec
        del whole, windowed
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--lone", type=int, default=20_000, help="items of the lone sequence")
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--window", type=int, default=20, help="window of the windowed evaluation beside it (step 1)")
    ap.add_argument("--labels", default="2,8,32")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for L in [int(x) for x in args.labels.split(",")]:
        line = json.dumps(run(L, args))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
