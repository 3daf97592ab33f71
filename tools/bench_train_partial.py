"""Partial-label training benchmark (a sibling of tools/bench_train_sequences.py): one objective + gradient evaluation of a
partially labelled problem per label count, as whole sequences (gecco_crf_trainer_sequences_create_partial) and as windows
(gecco_crf_trainer_general_create_partial, W = 20, step 1), and the labelled evaluation of the same items.

    python tools/bench_train_partial.py [--mode both|labelled] [--sequences 1000] [--length 200] [--labels 2,8,32] [--out FILE]

Half the items (seeded) carry a two-label set, {truth, one other label}; the others name their label.  ``--mode labelled``
times the labelled evaluation alone and uses nothing a commit without the partial creates lacks, so the same file measures
the parent commit on the same items.  Per label count it prints one JSON line; times are taken as in
tools/bench_train_sequences.py (host clock and two HIP events on the null stream around the synchronous call)."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import _native, synth  # noqa: E402
from bench_train_sequences import labelled_set, timed  # noqa: E402  (this directory)


def run(L, args):
    rng = np.random.default_rng(synth.SEED + L)
    A = args.attrs
    K = A * L + L * L
    sfid, tfid = np.arange(A * L, dtype=np.int32), A * L + np.arange(L * L, dtype=np.int32)
    w = rng.normal(0, 0.5, size=K)
    seq_ptr, item_ptr, attr_id, labels = labelled_set(rng, [args.length] * args.sequences, A, L)
    n = int(seq_ptr[-1])
    hidden = rng.random(n) < 0.5
    other = (labels + rng.integers(1, L, size=n)) % L
    masks = (np.uint64(1) << labels.astype(np.uint64))
    masks = np.where(hidden, masks | (np.uint64(1) << other.astype(np.uint64)), masks).astype(np.uint32)
    out = {"tool": "bench_train_partial", "mode": args.mode, "abi": int(_native.load_library().gecco_crf_version()), "labels": L,
           "attrs": A, "features": K, "items": n, "sequences": args.sequences, "hidden_items": int(hidden.sum())}
    problem = (seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K)
    for name, family, p in (("whole", _native.TrainerSequences, problem),
                            ("windowed", _native.TrainerGeneral, problem + (args.window, 1))):
        rec = {}
        tr = family([p])
        f, _ = tr.eval([w])
        rec["labelled"] = dict(timed(lambda: tr.eval([w]), args.warmup, args.evals), f=float(f[0]), scratch_bytes=tr.scratch_bytes(0))
        del tr
        if args.mode == "both":
            tr = family([p], allowed=[masks])
            f, _ = tr.eval([w])
            rec["partial"] = dict(timed(lambda: tr.eval([w]), args.warmup, args.evals), f=float(f[0]),
                                  scratch_bytes=tr.scratch_bytes(0))
            rec["partial_over_labelled"] = rec["partial"]["hip_event_us"][0] / rec["labelled"]["hip_event_us"][0]
            del tr
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("both", "labelled"), default="both")
    ap.add_argument("--sequences", type=int, default=1000)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--window", type=int, default=20, help="window of the windowed evaluation (step 1)")
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
