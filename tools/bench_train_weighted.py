"""Cost-sensitive training benchmark (a sibling of tools/bench_train_partial.py): one objective + gradient evaluation per
label count, as whole sequences (gecco_crf_trainer_sequences_*) and as windows (gecco_crf_trainer_general_*, W = 20, step 1),
of the unweighted problem, of the same problem with sequence weights, and with weights and a label-cost matrix.

    python tools/bench_train_weighted.py [--mode all|unweighted] [--sequences 1000] [--length 200] [--labels 2,8,32] [--out FILE]

The weights are seeded in [0.25, 4], the costs in [0, 2] with a zero diagonal.  ``--mode unweighted`` times the unweighted
evaluation alone and uses nothing a commit without the weighted creates lacks, so the same file, copied into a checkout of the
parent commit, measures that commit on the same items: case (a) beside this build's (b), which is the same machine code
(tools/isa_same.py).  At 2 labels the windowed problem is also timed on the 2-label trainer (gecco_crf_trainer_*), which a
weighted 2-label set no longer uses.  Per label count it prints one JSON line; times are taken as in
tools/bench_train_sequences.py (host clock and two HIP events on the null stream around the synchronous call; median, minimum
and maximum of the timed evaluations)."""
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
    weights = rng.uniform(0.25, 4.0, size=args.sequences)
    costs = rng.uniform(0.0, 2.0, size=(L, L))
    costs[np.arange(L), np.arange(L)] = 0.0
    out = {"tool": "bench_train_weighted", "mode": args.mode, "abi": int(_native.load_library().gecco_crf_version()), "labels": L,
           "attrs": A, "features": K, "items": int(seq_ptr[-1]), "sequences": args.sequences}
    problem = (seq_ptr, item_ptr, attr_id, labels, A, sfid, tfid, K)
    cases = [("unweighted", {})]
    if args.mode == "all":
        cases += [("weights", {"weights": [weights]}), ("weights_and_costs", {"weights": [weights], "costs": [costs]})]
    for name, family, p in (("whole", _native.TrainerSequences, problem),
                            ("windowed", _native.TrainerGeneral, problem + (args.window, 1))):
        rec = {}
        for case, kw in cases:
            tr = family([p], **kw)
            f, _ = tr.eval([w])
            rec[case] = dict(timed(lambda: tr.eval([w]), args.warmup, args.evals), f=float(f[0]), scratch_bytes=tr.scratch_bytes(0))
            del tr
        for case, _ in cases[1:]:
            rec[case + "_over_unweighted"] = rec[case]["hip_event_us"][0] / rec["unweighted"]["hip_event_us"][0]
        if L == 2 and name == "windowed":  # the trainer a weighted 2-label windowed set no longer uses
            tr = _native.Trainer(seq_ptr, item_ptr, attr_id, labels, A, args.window, 1, sfid, tfid, K)
            f, _ = tr.eval(w)
            rec["two_label_trainer"] = dict(timed(lambda: tr.eval(w), args.warmup, args.evals), f=float(f))
            for case, _ in cases[1:]:
                rec[case + "_over_two_label_trainer"] = rec[case]["hip_event_us"][0] / rec["two_label_trainer"]["hip_event_us"][0]
            del tr
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("all", "unweighted"), default="all")
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
