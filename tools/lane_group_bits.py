"""Bits of the any-label entries whose kernels share crf_lane_group.hpp, on a fixed, seeded grid of small batches: one line per
case with the SHA-256 of all output bytes of the call.  Built like tools/walk_bits.py.

    python tools/lane_group_bits.py [--out FILE] [--blocks FILE]
    python tools/lane_group_bits.py --condense FILE      (no device: the --blocks form of an --out file, on stdout)

Two builds of the library compute the same bits exactly when their outputs are the same file (GECCO_CRF_LIBRARY selects the
build).  tools/isa_same.py compares the kernels' machine code; this is for the host side, which it cannot see: block counts,
launcher picks, argument order.  The only atomics of these kernels write counters and the maxima of gl_windowed, both
order-independent.  `--blocks` writes the short form kept under profiles/: one line per block of cases (a label count or a
special family, and an entry) with the number of cases and the SHA-256 of the block's case lines.

The grid: label counts 2 (under GECCO_CRF_FORCE_GENERAL=1), 3, 5, 8, 9, 17, 32 (every group size LP, and L < LP); batches of
256 / LP + 1 contigs or queries (a second workgroup, almost empty), as many batches as it takes to hold contigs of 0, 1, 2, 31, 32,
33, 63, 64, 65 and 129 genes (around the back-pointer rows staged at a time, the two chunk lengths and twice the longer one: two
batches at 17 and 32 labels, one below); every whole-contig and query entry behind the recursions contig by contig
(GECCO_CRF_GENERAL_CHUNKED=0), chunked (=1) and in chunks of four genes (GECCO_CRF_GENERAL_CHUNK=4), and from nine labels behind
GECCO_CRF_GENERAL_MARGINALS / _VITERBI = chunked and split; the windowed entries on the lane-group tier
(GECCO_CRF_GENERAL_GROUPS=1) at windows of 5 and 20 and steps 1 and 3; and per special family (3 and 17 labels, the same
arrangements) valued batches, batches with `allowed` masks and an all-zero model, in which every comparison is a tie and every
chunked contig is decoded again.  A call that raises ends the run: a digest in the record always stands for output bytes."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch  # noqa: F401  (before libgecco_crf.so: the wheel's own libamdhip64 has to be the first one loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gecco_amd import _native, synth  # noqa: E402
from walk_bits import digest  # noqa: E402

LABELS = (2, 3, 5, 8, 9, 17, 32)
LENGTHS = (33, 0, 64, 1, 129, 2, 31, 65, 32, 63)
ATTRS = 40
SWITCHES = ("GECCO_CRF_GENERAL_CHUNKED", "GECCO_CRF_GENERAL_CHUNK", "GECCO_CRF_GENERAL_MARGINALS", "GECCO_CRF_GENERAL_VITERBI",
            "GECCO_CRF_GENERAL_GROUPS", "GECCO_CRF_FORCE_GENERAL")


ENTRIES = ("viterbi", "marginals_full", "span_log_probabilities", "run_posteriors", "edge_posteriors", "windowed_marginals",
           "windowed_marginals_all")


def blocks(lines):
    """The short form of the case lines: per block (a label count or family, and an entry) the cases and their digest."""
    order, groups = [], {}
    for line in lines:
        words = [w for w in line.split(" ") if not w.startswith("batch=")]
        key = " ".join(words[:next(i for i, w in enumerate(words) if w in ENTRIES) + 1])
        if key not in groups:
            order.append(key)
            groups[key] = []
        groups[key].append(line)
    return [f"{key} | cases {len(groups[key])} | sha256 {hashlib.sha256(chr(10).join(groups[key]).encode()).hexdigest()}" for key in order]


def arrangement(L, **switches):
    """Set the switches of one arrangement (the library reads them at every call) and return its name."""
    for name in SWITCHES:
        os.environ.pop(name, None)
    if L == 2:
        os.environ["GECCO_CRF_FORCE_GENERAL"] = "1"
    for key, value in switches.items():
        os.environ["GECCO_CRF_GENERAL_" + key] = str(value)
    return ",".join(f"{k.lower()}={v}" for k, v in switches.items()) or "default"


def recursions(L):
    yield {"CHUNKED": 0}
    yield {"CHUNKED": 1}
    yield {"CHUNKED": 1, "CHUNK": 4}
    if L >= 9:
        yield {"MARGINALS": "chunked", "VITERBI": "chunked"}
        yield {"MARGINALS": "split", "VITERBI": "split"}


def dict_digest(out):
    return digest(*(out[k] for k in sorted(out)))


def queries(rng, batch, L, n):
    """n spans, anchors and closed runs on the contigs that have genes, and three label sets."""
    lens = np.diff(batch[0])
    full = np.flatnonzero(lens > 0)
    c = full[np.arange(n) % full.size].astype(np.int32)
    a = (rng.integers(0, 1 << 30, size=n) % lens[c]).astype(np.int32)
    b = np.minimum(a + 1 + rng.integers(0, 40, size=n), lens[c]).astype(np.int32)
    every = (1 << L) - 1
    masks = np.array([(1 << (L // 2), every, every & 0x55555555)[i % 3] for i in range(n)], dtype=np.uint32)
    return c, a, b, masks, np.array([1 << (L // 2), every & 0x55555555, every & ~1 or 1], dtype=np.uint32)


def entry_cases(name, model, batch, L, rng, values=None, allowed=None):
    kw = {"values": values, "allowed": allowed}
    lp = max(2, 1 << (L - 1).bit_length())
    c, a, b, masks, sets = queries(rng, batch, L, 256 // lp + 1)
    for rec in recursions(L):
        arr = arrangement(L, **rec)
        for want in (True, False):
            yield f"{name} viterbi {arr} score={int(want)}", digest(*model.viterbi(*batch, want_score=want, **kw))
        yield f"{name} marginals_full {arr}", digest(*model.marginals_full(*batch, **kw))
        yield f"{name} span_log_probabilities {arr}", digest(model.span_log_probabilities(*batch, c, a, b, masks, **kw))
        for reach in (0, 3):
            yield f"{name} run_posteriors {arr} reach={reach}", dict_digest(model.run_posteriors(*batch, anchors=(c, a, masks), reach=reach, **kw))
        yield f"{name} run_posteriors {arr} closed", dict_digest(model.run_posteriors(*batch, runs=(c, a, b, masks), **kw))
        yield f"{name} edge_posteriors {arr}", dict_digest(model.edge_posteriors(*batch, sets=sets, want_pair=True, **kw))
    arr = arrangement(L, GROUPS=1)
    for window in (5, 20):
        for step in (1, 3):
            tail = f"{arr} W={window} step={step}"
            yield f"{name} windowed_marginals {tail}", digest(model.windowed_marginals(*batch, window, step=step, label=1, **kw))
            yield f"{name} windowed_marginals_all {tail}", digest(*model.windowed_marginals_all(*batch, window, step=step, background=0, **kw))
    arrangement(0)


def batches(rng, L, shift=0):
    """Batches of 256 / LP + 1 contigs that between them hold every length of LENGTHS (one batch where it holds ten contigs)."""
    lp = max(2, 1 << (L - 1).bit_length())
    n = 256 // lp + 1
    for start in range(0, len(LENGTHS), n):
        yield synth.synth_contigs(rng, [LENGTHS[(shift + start + i) % len(LENGTHS)] for i in range(n)], ATTRS)


def cases():
    for L in LABELS:
        rng = np.random.default_rng(synth.SEED + 500 * L)
        model = _native.Model.from_tables(rng.normal(0, 0.5, size=(ATTRS, L)), rng.normal(0, 0.5, size=(L, L)))
        for b, batch in enumerate(batches(rng, L)):
            yield from entry_cases(f"L={L} batch={b}", model, batch, L, rng)
    for L in (3, 17):
        rng = np.random.default_rng(synth.SEED + 7000 + L)
        model = _native.Model.from_tables(rng.normal(0, 0.5, size=(ATTRS, L)), rng.normal(0, 0.5, size=(L, L)))
        zero = _native.Model.from_tables(np.zeros((ATTRS, L)), np.zeros((L, L)))
        for b, batch in enumerate(batches(rng, L, shift=3)):
            n = int(batch[0][-1])
            values = rng.uniform(0.25, 4.0, size=batch[2].size)
            yield from entry_cases(f"valued L={L} batch={b}", model, batch, L, rng, values=values)
            allowed = rng.integers(1, 1 << L, size=n, dtype=np.uint64).astype(np.uint32) | np.uint32(1 << (L // 2))
            yield from entry_cases(f"masked L={L} batch={b}", model, batch, L, rng, allowed=allowed)
            yield from entry_cases(f"ties L={L} batch={b}", zero, batch, L, rng)


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
