"""Cross-validation training benchmark (not bench.py): the K folds of a synthetic labelled set fitted in one batch
(train.fit_training_sets, one batched objective per round) against the same folds fitted one after another
(train.fit_training_set).

    python tools/bench_cv.py [--items 200000,1000000] [--folds 5,10] [--window 5] [--max-iterations 100] [--out FILE]

Per (items, K) it prints one JSON line: the wall time of both (trainer creation included), the batched evaluations per
second (fold evaluations done / batched wall time), the rounds (batched evaluations) against the sequential fits' sum of
evaluations, and whether every fold's result is bitwise the sequential one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import synth, train  # noqa: E402
from gecco_amd.cv import kfold_splits  # noqa: E402


def fold_sets(seq_ptr, item_ptr, attr_id, labels, A, k, window):
    """The training set of every fold of kfold_splits over the sequences, with every (attribute, label) pair and every
    transition as a feature."""
    sets = []
    n_seqs, n_items = len(seq_ptr) - 1, int(seq_ptr[-1])
    owner_seq = np.repeat(np.arange(n_seqs), np.diff(seq_ptr))
    owner_item = np.repeat(np.arange(n_items), np.diff(item_ptr))
    for train_idx, _ in kfold_splits(n_seqs, k):
        keep_seq = np.zeros(n_seqs, dtype=bool)
        keep_seq[train_idx] = True
        keep = keep_seq[owner_seq]
        items = np.flatnonzero(keep)
        lens = np.diff(seq_ptr)[train_idx]
        deg = np.diff(item_ptr)[items]
        attr = attr_id[keep[owner_item]]
        sets.append(train.TrainingSet(
            seq_ptr=np.r_[0, np.cumsum(lens)].astype(np.int32), item_ptr=np.r_[0, np.cumsum(deg)].astype(np.int32),
            attr_id=attr.astype(np.int32), labels=labels[items].astype(np.int32), labels_=["0", "1"],
            attrs_=[f"a{a}" for a in range(A)], state_attr=np.repeat(np.arange(A), 2), state_label=np.tile([0, 1], A),
            trans_src=np.array([0, 0, 1, 1]), trans_dst=np.array([0, 1, 0, 1]),
            state_fid=np.arange(2 * A, dtype=np.int32).reshape(A, 2),
            trans_fid=(2 * A + np.arange(4, dtype=np.int32)).reshape(2, 2), window=window, step=1))
    return sets


def run(n_items, k, args):
    rng = np.random.default_rng(synth.SEED + n_items + k)
    lengths = np.maximum(synth.contig_lengths(rng, max(1, n_items // 200), total_genes=n_items), args.window)
    seq_ptr, item_ptr, attr_id, labels = synth.synth_training_set(rng, lengths, args.attrs)
    sets = fold_sets(seq_ptr, item_ptr, attr_id, labels, args.attrs, k, args.window)
    params = train.trainer_params({"c1": args.c1, "c2": args.c2, "max_iterations": args.max_iterations})
    train.fit_training_set(sets[0], train.trainer_params({"max_iterations": 1}))  # (warm-up: library, device)
    t0 = time.perf_counter()
    seq = [train.fit_training_set(ts, params) for ts in sets]
    t_seq = time.perf_counter() - t0
    t0 = time.perf_counter()
    bat = train.fit_training_sets(sets, params)
    t_bat = time.perf_counter() - t0
    same = all(a.x.tobytes() == b.x.tobytes() and (a.n_iter, a.n_eval, a.status) == (b.n_iter, b.n_eval, b.status)
               for a, b in zip(seq, bat))
    evals = sum(r.n_eval for r in bat)
    return {"bench": "cv_train", "items": int(seq_ptr[-1]), "folds": k, "window": args.window, "attrs": args.attrs,
            "fold_items": [int(ts.seq_ptr[-1]) for ts in sets],
            "sequential_s": t_seq, "batched_s": t_bat, "speedup": t_seq / t_bat,
            "fold_evals": evals, "batched_rounds": max(r.n_eval for r in bat), "batched_evals_per_s": evals / t_bat,
            "n_iter": [r.n_iter for r in bat], "bitwise_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", default="200000,1000000")
    ap.add_argument("--folds", default="5,10")
    ap.add_argument("--attrs", type=int, default=2766)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--c1", type=float, default=0.15)
    ap.add_argument("--c2", type=float, default=0.15)
    ap.add_argument("--max-iterations", type=int, default=100)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for n in (int(x) for x in args.items.split(",")):
        for k in (int(x) for x in args.folds.split(",")):
            line = json.dumps(run(n, k, args))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
