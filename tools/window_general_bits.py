"""Bits of the any-label window kernels on a fixed, seeded grid of small batches: one line per case with the SHA-256 of the
output bytes (gecco_crf_windowed_marginals, gecco_crf_windowed_marginals_all and their valued forms; four whole-contig cases
and the plan entry beside them).

    python tools/window_general_bits.py [--out FILE] [--blocks FILE]
    python tools/window_general_bits.py --condense FILE      (no device: the --blocks form of an --out file, on stdout)

Two builds of the library compute the same bits exactly when their outputs are the same file (GECCO_CRF_LIBRARY selects the
build).  `--blocks` writes the short form that is kept under profiles/: one line per block of cases (a label count and a
window, or one of the special families) with the number of cases and the SHA-256 of the block's case lines, so two short
files are equal exactly when the long ones are.

The grid holds the smallest shapes at which the kernels of crf_general_windowed.hip take another path:
label counts 1, 2, 3, 5, 8, 9, 17, 32 (every group size LP, L < LP with idle lanes, both sides of the lane-per-window tier's
limit and of the matrix-core tier's lower limit; the 2-label single-label passes run under GECCO_CRF_FORCE_GENERAL);
windows of 1, 2, 5, 20, 21, 32, 33 and 48 genes (the WMAX = 20 / 32 boundaries, the limit of 20 beyond 4 labels, the lane-group
tier's longest window) at step 1 and step 3, padded and not; contigs of 1 gene, of W - 1, W and W + 3 genes and one of two
tiles and a part (256 - (W - 1) slots per tile: carries between waves and tiles, a partly empty last tile) -- without padding
the short ones are skipped (NaN, and a gap in the gene numbering: an irregular tile), with padding they are padded; one
label at a time for labels 0, L // 2 and L - 1, and every label with no background, background 0 and background L - 1; each
with GECCO_CRF_GENERAL_GROUPS unset and set; transition spreads of 31.5 and 31.6 at W = 20 (inside and outside the range
guard); one valued case per entry; marginals_full and viterbi at 3 and 17 labels; and the all-label entry on a plan that has
run a whole-contig pass."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import _native, synth  # noqa: E402

LABELS = (1, 2, 3, 5, 8, 9, 17, 32)
WINDOWS = (1, 2, 5, 20, 21, 32, 33, 48)
ATTRS = 60
GROUPS, FORCE = "GECCO_CRF_GENERAL_GROUPS", "GECCO_CRF_FORCE_GENERAL"


def lengths(W):
    return [1, W - 1, W, 2 * (256 - (W - 1)) + 57, W + 3, 1]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def env(name, on):
    if on:
        os.environ[name] = "1"
    else:
        os.environ.pop(name, None)


def window_cases(name, model, L, batch, W, step, pad, values=None):
    """Every single-label and all-label pass of one batch, in both tiers: (name, digest, NaN count)."""
    cptr, gptr, attr = batch
    for groups in (False, True):
        env(GROUPS, groups)
        tier = "groups" if groups else "auto"
        env(FORCE, L == 2)  # (a 2-label model takes the any-label kernels only when told to)
        for label in sorted({0, L // 2, L - 1}):
            p = model.windowed_marginals(cptr, gptr, attr, W, step, label, pad, values=values)
            yield f"{name} {tier} label={label}", digest(p), int(np.isnan(p).sum())
        env(FORCE, False)
        for bg in (None,) + tuple(sorted({0, L - 1})):
            p_all, p_any = model.windowed_marginals_all(cptr, gptr, attr, W, step, background=bg, pad=pad, values=values)
            yield f"{name} {tier} all background={bg}", digest(p_all, p_any), int(np.isnan(p_all).sum())
    env(GROUPS, False)


def cases():
    for L in LABELS:
        rng = np.random.default_rng(synth.SEED + 100 * L)
        model = _native.Model.from_tables(rng.normal(0, 0.5, size=(ATTRS, L)), rng.normal(0, 0.5, size=(L, L)))
        for W in WINDOWS:
            batch = synth.synth_contigs(rng, lengths(W), ATTRS)
            for step in sorted({1, min(3, W)}):
                for pad in (True, False):
                    yield from window_cases(f"L={L} W={W} step={step} pad={int(pad)}", model, L, batch, W, step, pad)
    # the range guard of the tile kernels: (W - 1) * spread < 600, the construction of tests/test_gpu_general.py
    rng = np.random.default_rng(77)
    L, W = 3, 20
    w = np.clip(rng.laplace(0.0, 6.0, size=(ATTRS, L)), -40.0, 40.0)
    batch = synth.synth_contigs(rng, lengths(W), ATTRS)
    for spread in (31.5, 31.6):
        trans = rng.uniform(-1.0, 1.0, size=(L, L))
        trans[1, 2] = trans.max() - spread
        trans[trans < trans[1, 2]] = trans[1, 2]
        model = _native.Model.from_tables(w, trans)
        yield from window_cases(f"spread={spread} L=3 W=20 step=1 pad=1", model, L, batch, W, 1, True)
    # attribute values (both entries go through the valued state scores), and the whole-contig recursions beside them
    for L in (3, 17):
        rng = np.random.default_rng(synth.SEED + 7000 + L)
        model = _native.Model.from_tables(rng.normal(0, 0.5, size=(ATTRS, L)), rng.normal(0, 0.5, size=(L, L)))
        batch = synth.synth_contigs(rng, lengths(20), ATTRS)
        values = rng.uniform(0.25, 4.0, size=batch[2].size)
        yield from window_cases(f"valued L={L} W=20 step=1 pad=1", model, L, batch, 20, 1, True, values=values)
        marg, lognorm = model.marginals_full(*batch)
        yield f"marginals_full L={L}", digest(marg, lognorm), 0
        y, score = model.viterbi(*batch)
        yield f"viterbi L={L}", digest(y, score), 0
    # the all-label entry on a plan laid out for another geometry, after a whole-contig pass on that plan
    for L, pad in ((2, True), (2, False), (3, False)):
        rng = np.random.default_rng(synth.SEED + 8000 + L)
        model = _native.Model.from_tables(rng.normal(0, 0.5, size=(ATTRS, L)), rng.normal(0, 0.5, size=(L, L)))
        cptr, gptr, attr = synth.synth_contigs(rng, [3, 300, 0, 7, 19, 600, 12, 45, 1, 260, 5], ATTRS)
        n = int(cptr[-1])
        env(GROUPS, L != 2)
        plan = _native.Plan(model, cptr, 20, 1, pad, device=0)
        env(GROUPS, False)
        dev = torch.device("cuda:0")
        d_gp, d_at = torch.from_numpy(np.asarray(gptr, dtype=np.int32)).to(dev), torch.from_numpy(np.asarray(attr, dtype=np.int32)).to(dev)
        y = torch.zeros(n, dtype=torch.int8, device=dev)
        p_all = torch.full((n, L), -1.0, dtype=torch.float64, device=dev)
        p_any = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        plan.run_viterbi(d_gp.data_ptr(), d_at.data_ptr(), y.data_ptr())
        plan.run_windowed_all(d_gp.data_ptr(), d_at.data_ptr(), p_all.data_ptr(), p_any.data_ptr(), background=0)
        torch.cuda.synchronize()
        out = p_all.cpu().numpy()
        yield f"plan after viterbi L={L} pad={int(pad)} {plan.all_kernel_name}", digest(out, p_any.cpu().numpy(), y.cpu().numpy()), int(np.isnan(out).sum())
        del plan


def blocks(lines):
    """The short form of the case lines: per block (the case name up to its step, or its first word) the cases and their digest."""
    order, groups = [], {}
    for line in lines:
        name = line.split(" | ")[0]
        key = name.split(" step=")[0] if name.startswith("L=") else name.split(" L=")[0]
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
    for name, sha, nans in cases():
        lines.append(f"{name} | NaN {nans} | sha256 {sha}")
        print(lines[-1], flush=True)
    for path, text in ((args.out, lines), (args.blocks, blocks(lines))):
        if path:
            with open(path, "w") as fh:
                fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
