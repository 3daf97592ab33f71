"""Bits of the general and whole-sequence trainers on a fixed, seeded grid of small problems: one line per case with the
SHA-256 of the bytes of f and g (gecco_crf_trainer_general_eval, gecco_crf_trainer_sequences_eval).

    python tools/train_general_bits.py [--out FILE]

Two builds of the library compute the same bits exactly when their outputs are the same file (GECCO_CRF_LIBRARY selects the
build).  The grid holds the smallest shapes at which the instance kernels of crf_train_general.hip take another path:
label counts 2, 3, 5, 8, 9, 17, 32 (every group size G, and L < G with idle lanes); windows of 1, 2, 5 and 20 items at step
1 and at a step above 1, 300 windows (more than one workgroup of 128, the last one partly empty); 150 whole sequences of
1, 2 and up to 60 items (more than 256 / G for every G, and no multiple of it); each labelled and with allowed-label masks
(singleton, multi-label and all-label), once per family with attribute values, once with transitions 700 apart, and two
problems in one trainer with one of them inactive."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import _native, synth  # noqa: E402

LABELS = (2, 3, 5, 8, 9, 17, 32)
WINDOWS = ((1, 1), (2, 1), (2, 2), (5, 1), (5, 3), (20, 1), (20, 3))  # (window, step)
ATTRS = 40


def problem(rng, lengths, L):
    """(seq_ptr, item_ptr, attr_id, labels, A, state_fid, trans_fid, K) with every feature present, and its item count."""
    seq_ptr, item_ptr, attr_id = synth.synth_contigs(rng, lengths, ATTRS)
    n = int(seq_ptr[-1])
    labels = rng.integers(0, L, size=n).astype(np.int32)
    K = ATTRS * L + L * L
    sfid, tfid = np.arange(ATTRS * L, dtype=np.int32), ATTRS * L + np.arange(L * L, dtype=np.int32)
    return (seq_ptr.astype(np.int32), item_ptr.astype(np.int32), attr_id.astype(np.int32), labels, ATTRS, sfid, tfid, K), n


def window_lengths(W, step):
    """Three sequences of 97, 103 and 100 windows: 300 windows."""
    return [W + (c - 1) * step for c in (97, 103, 100)]


def sequence_lengths(rng):
    """150 sequences: lengths 1 and 2 among lengths up to 60."""
    lengths = rng.integers(1, 61, size=150)
    lengths[:6] = (1, 2, 60, 1, 2, 59)
    return [int(x) for x in lengths]


def masks_of(rng, labels, L):
    """A third of the items name their label, a third allow it and up to two others, a third allow every label."""
    n = labels.size
    kind = rng.integers(0, 3, size=n)
    m = np.uint64(1) << labels.astype(np.uint64)
    for _ in range(2):
        m = np.where(kind == 1, m | (np.uint64(1) << rng.integers(0, L, size=n).astype(np.uint64)), m)
    return np.where(kind == 2, np.uint64((1 << L) - 1), m).astype(np.uint32)


def digest(f, g):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(f, dtype=np.float64).tobytes())
    h.update(np.ascontiguousarray(g, dtype=np.float64).tobytes())
    return h.hexdigest()


def cases():
    """(name, family, problems, keyword arguments of the trainer, weights per problem, active mask or None)"""
    for L in LABELS:
        for W, step in WINDOWS:
            rng = np.random.default_rng(synth.SEED + 1000 * L + 10 * W + step)
            p, n = problem(rng, window_lengths(W, step), L)
            w = rng.normal(0, 0.5, size=p[7])
            yield f"windowed L={L} W={W} step={step} labelled", _native.TrainerGeneral, [p + (W, step)], {}, [w], None
            masks = masks_of(rng, p[3], L)
            yield (f"windowed L={L} W={W} step={step} partial", _native.TrainerGeneral, [p + (W, step)], {"allowed": [masks]},
                   [w], None)
        rng = np.random.default_rng(synth.SEED + 1000 * L + 7)
        p, n = problem(rng, sequence_lengths(rng), L)
        w = rng.normal(0, 0.5, size=p[7])
        yield f"whole L={L} labelled", _native.TrainerSequences, [p], {}, [w], None
        masks = masks_of(rng, p[3], L)
        yield f"whole L={L} partial", _native.TrainerSequences, [p], {"allowed": [masks]}, [w], None
    # attribute values, once per family; transitions 700 apart, once per family (labelled and partial)
    L = 9
    rng = np.random.default_rng(synth.SEED + 77)
    pw, _ = problem(rng, window_lengths(5, 3), L)
    ps, _ = problem(rng, sequence_lengths(rng), L)
    for name, family, p in (("windowed L=9 W=5 step=3", _native.TrainerGeneral, pw + (5, 3)), ("whole L=9", _native.TrainerSequences, ps)):
        w = rng.normal(0, 0.5, size=p[7])
        values = rng.uniform(0.25, 4.0, size=p[2].size)
        yield f"{name} valued", family, [p], {"values": [values]}, [w], None
        masks = masks_of(rng, p[3], L)
        yield f"{name} valued partial", family, [p], {"values": [values], "allowed": [masks]}, [w], None
        far = w.copy()
        far[ATTRS * L:] = np.where(rng.random(L * L) < 0.5, 350.0, -350.0)
        yield f"{name} transitions 700 apart", family, [p], {}, [far], None
        yield f"{name} transitions 700 apart partial", family, [p], {"allowed": [masks]}, [far], None
    # two problems in one trainer, labelled beside partial, both active and each alone
    rng = np.random.default_rng(synth.SEED + 78)
    for name, family, tail in (("windowed", _native.TrainerGeneral, lambda W, s: (W, s)), ("whole", _native.TrainerSequences, lambda W, s: ())):
        pa, _ = problem(rng, window_lengths(5, 1) if tail(5, 1) else sequence_lengths(rng), 3)
        pb, _ = problem(rng, window_lengths(20, 3) if tail(20, 3) else sequence_lengths(rng), 17)
        probs = [pa + tail(5, 1), pb + tail(20, 3)]
        ws = [rng.normal(0, 0.5, size=pa[7]), rng.normal(0, 0.5, size=pb[7])]
        allowed = [None, masks_of(rng, pb[3], 17)]
        for active in ([True, True], [True, False], [False, True]):
            yield f"{name} two problems L=3,17 active={active}", family, probs, {"allowed": allowed}, ws, active


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = []
    for name, family, probs, kw, ws, active in cases():
        tr = family(probs, **kw)
        f = np.full(len(probs), -1.0)  # (an inactive problem keeps what it had: its entries are part of the digest)
        g = [np.full(p[7], -1.0) for p in probs]
        tr.eval([w if (active is None or a) else None for w, a in zip(ws, active or [True] * len(ws))], active, f, g)
        if not all(np.isfinite(x).all() for x in [f] + g):
            raise SystemExit(f"{name}: a value that is not finite")
        instances = ",".join(str(tr.num_windows(k)) for k in range(len(probs)))
        lines.append(f"{name} | instances {instances} | f {' '.join(repr(float(x)) for x in f)} | sha256 {digest(f, np.concatenate(g))}")
        print(lines[-1], flush=True)
        del tr
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
