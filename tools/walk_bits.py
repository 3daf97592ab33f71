"""Bits of the whole-contig walks that share crf_contig_walk.hpp, on a fixed, seeded grid of small batches: one line per case with
the SHA-256 of all output bytes of the call (viterbi_kbest, viterbi_min_run, marginals_min_run, run_counts).

    python tools/walk_bits.py [--out FILE] [--blocks FILE]
    python tools/walk_bits.py --condense FILE      (no device: the --blocks form of an --out file, on stdout)

Two builds of the library compute the same bits exactly when their outputs are the same file (GECCO_CRF_LIBRARY selects the
build); the kernels use no atomics.  `--blocks` writes the short form that is kept under profiles/: one line per block of cases
(a label count and an entry, or one of the special families) with the number of cases and the SHA-256 of the block's case
lines, so two short files are equal exactly when the long ones are.

The grid holds the smallest shapes at which the frame can go wrong: label counts 2, 3, 5, 8, 9, 17, 32 (every group size LP,
and L < LP with idle lanes); k, min_run and max_runs of 1, 2, 3, 8, 31, 32 (both parities of the padded LDS row, K + 1 slots
for the counts, the degenerate rule at 1); batches of 64 / LP + 1 contigs (the last wave is partly empty) of 0, 1, 2, 8, 9, 10,
16, 17 and 18 genes, around the multiples of the eight-gene prefetch block that starts at gene 1, so that the groups of a wave
end at different genes; label sets of one label, every label and every second label; every entry with each of its optional
outputs alone and with all of them; and per special family a batch whose `allowed` masks leave the constrained entries
without a feasible path, a valued batch, and an all-zero model, in which every comparison is a tie."""
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
PARAMS = (1, 2, 3, 8, 31, 32)
LENGTHS = (9, 0, 17, 1, 8, 18, 2, 16, 10)
ATTRS = 40


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def batches(rng, L):
    """Batches of 64 / LP + 1 contigs that between them hold every length of LENGTHS."""
    lp = max(2, 1 << (L - 1).bit_length())
    n = 64 // lp + 1
    for start in range(0, len(LENGTHS), n):
        yield synth.synth_contigs(rng, [LENGTHS[(start + i) % len(LENGTHS)] for i in range(n)], ATTRS)


def sets(L):
    every = (1 << L) - 1
    return (("one", 1 << (L // 2)), ("every", every), ("second", every & 0x55555555))


def entry_cases(name, model, batch, L, params, values=None, allowed=None):
    """Every entry on one batch: (name, digest)."""
    kw = {"values": values, "allowed": allowed}
    for p in params:
        yield f"{name} viterbi_kbest p={p}", digest(*model.viterbi_kbest(*batch, p, **kw))
    for label, mask in sets(L):
        for p in params:
            tail = f"p={p} set={label}"
            for want in (True, False):
                yield f"{name} viterbi_min_run {tail} lognorm={int(want)}", digest(*model.viterbi_min_run(*batch, mask, p, want_lognorm=want, **kw))
            for marg, inside in ((True, False), (False, True), (True, True)):
                out = model.marginals_min_run(*batch, mask, p, want_marginals=marg, want_inside=inside, **kw)
                yield f"{name} marginals_min_run {tail} marg={int(marg)} inside={int(inside)}", digest(*out)
            for mass, paths in ((True, False), (False, True), (True, True)):
                out = model.run_counts(*batch, mask, p, want_log_mass=mass, want_paths=paths, **kw)
                yield f"{name} run_counts {tail} log_mass={int(mass)} paths={int(paths)}", digest(*out)


def cases():
    for L in LABELS:
        rng = np.random.default_rng(synth.SEED + 300 * L)
        model = _native.Model.from_tables(rng.normal(0, 0.5, size=(ATTRS, L)), rng.normal(0, 0.5, size=(L, L)))
        for b, batch in enumerate(batches(rng, L)):
            yield from entry_cases(f"L={L} batch={b}", model, batch, L, PARAMS)
    for L in (3, 17):
        rng = np.random.default_rng(synth.SEED + 9000 + L)
        model = _native.Model.from_tables(rng.normal(0, 0.5, size=(ATTRS, L)), rng.normal(0, 0.5, size=(L, L)))
        batch = next(batches(rng, 2))  # (33 contigs: every length, several waves)
        n = int(batch[0][-1])
        # genes take turns between label 0 alone and label 1 alone: every run of a set that holds one of the two has one gene,
        # so min_run >= 2 has no feasible path in a contig of two genes or more, and the run count of a contig is fixed
        allowed = np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.uint32)
        yield from entry_cases(f"infeasible L={L}", model, batch, L, (1, 2, 8), allowed=allowed)
        values = rng.uniform(0.25, 4.0, size=batch[2].size)
        yield from entry_cases(f"valued L={L}", model, batch, L, (1, 3, 32), values=values)
        zero = _native.Model.from_tables(np.zeros((ATTRS, L)), np.zeros((L, L)))
        yield from entry_cases(f"ties L={L}", zero, batch, L, (1, 2, 31))


def blocks(lines):
    """The short form of the case lines: per block (a label count or family, and an entry) the cases and their digest."""
    order, groups = [], {}
    for line in lines:
        words = line.split(" | ")[0].split(" ")
        key = " ".join(w for w in words[:4] if not w.startswith(("batch=", "p=", "set=")))
        if key not in groups:
            order.append(key)
            groups[key] = []
        groups[key].append(line)
    return [f"{key} | cases {len(groups[key])} | sha256 {hashlib.sha256(chr(10).join(groups[key]).encode()).hexdigest()}" for key in order]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the case lines to this file")
    ap.add_argument("--blocks", default=None, help="write the short form (one line per block of cases) to this file")
    ap.add_argument("--condense", default=None, metavar="FILE", help="print the short form of an --out file and exit (no device)")
    args = ap.parse_args()
    if args.condense:
        with open(args.condense) as fh:
            print("\n".join(blocks([line.rstrip("\n") for line in fh if line.strip()])))
        return
    lines = []
    for name, sha in cases():
        lines.append(f"{name} | sha256 {sha}")
        print(lines[-1], flush=True)
    for path, text in ((args.out, lines), (args.blocks, blocks(lines))):
        if path:
            with open(path, "w") as fh:
                fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
