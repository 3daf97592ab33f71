#!/usr/bin/env python3
"""profiles/MEASUREMENTS.md from the committed records of the round (profiles/r06_*): every number in that file is read from the
file it names, so the document cannot drift from the records.   usage: python tools/measurements_md.py > profiles/MEASUREMENTS.md
(the head of the file, §1 to §7); python tools/measurements_md.py --section 7m prints §7m from profiles/runs_bench.jsonl,
--section 7n prints §7n from profiles/minrun_marginals_bench.jsonl, --section 7o prints §7o from profiles/counts_bench.jsonl,
--section walk prints the contig-walk refactor's section from profiles/walk_refactor_ab.txt and profiles/walk_bits.txt."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = os.path.join(ROOT, "profiles")
TAG = "r06"


def J(name):
    with open(os.path.join(P, f"{TAG}_{name}.json")) as fh:
        return json.load(fh)


def us(ms):
    return ms * 1e3


def sci(x):
    e = len(str(int(x))) - 1
    sup = str(e).translate(str.maketrans("0123456789", "⁰¹²³⁴⁵⁶⁷⁸⁹"))
    return f"{x / 10 ** e:.1f}·10{sup}"


def kt(summary, prefix, kernel):
    """calls, avg_us of `kernel` in the trace `prefix` of a prof_summary.py text"""
    for line in summary.splitlines():
        if line.startswith(prefix) and "KERNEL" in line and kernel in line:
            return int(re.search(r"calls=(\d+)", line).group(1)), float(re.search(r"avg_us=([\d.]+)", line).group(1))
    return None, None


def section_7m():
    """§7m from profiles/runs_bench.jsonl and profiles/runs_kernel_stats.txt (``python tools/measurements_md.py --section 7m``):
    the section is appended to MEASUREMENTS.md behind §7l, like its neighbours, which describe later work than the round's set."""
    rows = [json.loads(ln) for ln in open(os.path.join(P, "runs_bench.jsonl")) if ln.strip()]
    stats, reach = {}, None
    for ln in open(os.path.join(P, "runs_kernel_stats.txt")):
        if ln.startswith("== reach"):
            reach = int(ln.split()[2])
        m = re.match(r'"void gecco::\(anonymous namespace\)::gl_run_walk<(\d+), (true|false)>[^"]*",(\d+),(\d+),([\d.]+),[\d.]+,(\d+),(\d+)', ln)
        if m:
            stats[(reach, int(m.group(1)), m.group(2) == "true")] = int(m.group(7)) / 1e3  # the largest launch: all the anchors
    t0 = rows[0]
    reaches = t0["reaches"]
    fmt = lambda v: f"{v['hip_event_us'][0]:.0f} ({v['hip_event_us'][1]:.0f} – {v['hip_event_us'][2]:.0f})"
    out = []
    A = out.append
    A("### 7m. Run posteriors: `gecco_crf_run_posteriors` (`tools/bench_runs.py`, `runs_bench.jsonl`, `runs_kernel_stats.txt`)\n")
    A(f"One `Model.run_posteriors` call (DESIGN.md §4.9l) with {t0['anchors']} anchors (uniform sequences and items, random proper label "
      f"sets) at reach {' / '.join(str(r) for r in reaches)} on §7g's batch: {t0['sequences']} sequences of {t0['items'] // t0['sequences']} items, "
      f"{t0['items']} items, about {t0['entries']} attribute entries, weights N(0, 0.5), at {' / '.join(str(t['labels']) for t in rows)} labels, no "
      "marginals asked for.  Beside it, in the same rounds: the same entry with ONE anchor at reach 0 (the pass alone, as this entry runs "
      "it: any-L kernels, nothing per item brought back); one closed-run query per anchor instead of the anchors; `Model.marginals_full` "
      "as a caller gets it and through the any-L kernels; and the route the exact distributions replace, `Model.sample_paths` with the same "
      f"anchors as run queries at N = {t0['samples']} paths kept on the device.  Times are two HIP events on the null stream around the "
      f"synchronous one-shot call (plan build, upload, launches, download), {t0['warmup']} warm-up rounds, median of {t0['evals_timed']} "
      "(minimum – maximum), the calls in turn inside every round.\n")
    A("| L | " + " | ".join(f"reach {r}, µs" for r in reaches) + " | closed runs, µs | pass alone (one anchor), µs | `marginals_full` / any-L, µs | `sample_paths` + runs, N = "
      f"{t0['samples']}, µs |")
    A("|---" * (len(reaches) + 5) + "|")
    for t in rows:
        A(f"| {t['labels']} | " + " | ".join(fmt(t[f"runs_reach_{r}"]) for r in reaches) + f" | {fmt(t['runs_closed'])} | {fmt(t['pass_one_anchor'])} | "
          f"{t['marginals_full']['hip_event_us'][0]:.0f} / {t['marginals_full_any_l']['hip_event_us'][0]:.0f} | {fmt(t['sample_runs'])} |")
    A("")
    A("The two walk launches alone, from a kernel trace in a run of its own (`rocprofv3 --kernel-trace --stats`, one traced run of the "
      "tool per reach with 10 timed rounds; the duration of the longest launch of each kernel, which is a launch with all the anchors -- "
      "the kernels also serve the one-anchor and closed-run calls of the tool):\n")
    A("| L | " + " | ".join(f"reach {r}: left + right walks, µs" for r in reaches) + " |")
    A("|---" * (len(reaches) + 1) + "|")
    lp = lambda L: 2 if L <= 2 else 4 if L <= 4 else 8 if L <= 8 else 16 if L <= 16 else 32
    for t in rows:
        A(f"| {t['labels']} | " + " | ".join(f"{stats[(r, lp(t['labels']), False)]:.0f} + {stats[(r, lp(t['labels']), True)]:.0f}" for r in reaches) + " |")
    A("")
    A("What the figures say, and what they do not:\n")
    A("* The call's time over the pass alone (" + "; ".join(
        f"{t['labels']} labels: " + " / ".join(f"{t['walks_us'][str(r)]:.0f}" for r in reaches) for t in rows) + " µs at reach " +
      " / ".join(str(r) for r in reaches) + ") is the two launches AND the download of 2 · anchors · (reach + 1) doubles to pageable memory "
      f"({2 * t0['anchors'] * (reaches[-1] + 1) * 8 / 1e6:.1f} MB at reach {reaches[-1]}); the trace separates the launches.  A walk is sequential: its "
      "time is a chain of reach + 2 steps of dependent reductions, " +
      f"{min(stats[(reaches[-1], lp(t['labels']), False)] for t in rows) / reaches[-1]:.1f} – {max(stats[(reaches[-1], lp(t['labels']), side)] for t in rows for side in (False, True)) / reaches[-1]:.1f} µs a step at reach {reaches[-1]}, and 1 000 walks do not fill the device.  The "
      "closed runs (five items each) are within the noise of the pass alone.")
    A("* Against the sampled route the exact call takes " + "; ".join(
        f"{t['labels']} labels: " + " / ".join(f"{t['runs_over_sample_runs'][str(r)]:.2f}" for r in reaches) for t in rows) +
      f" of its time at reach {' / '.join(str(r) for r in reaches)}, and answers what N = {t0['samples']} paths cannot: of the "
      f"{t0['finite_entries']} finite start and end entries at reach {reaches[-1]}, " +
      " / ".join(str(t["entries_below_1_over_samples"]) for t in rows) + f" have a probability below 1 / N, down to log p = " +
      " / ".join(f"{t['min_finite_log_p']:.0f}" for t in rows) + ".  The sampled share of paths with the anchor in the set agrees with "
      "exp(log_anchor) to " + " / ".join(f"{t['sampled_vs_exact']['max_abs_difference']:.3f}" for t in rows) + " at the worst anchor (" +
      " / ".join(f"{t['sampled_vs_exact']['max_in_sigma']:.1f}" for t in rows) + " σ).")
    A("* Accuracy, from `tests/test_gpu_runs.py` on an MI355X (yardstick: log Z_A′ − log Z_A in numpy log space; bound: 1e-10 (max(1, "
      "|log Z_A′|) + max(1, |log Z_A|)) per entry): worst difference / bound 3.8e-5 over the twenty (label count, kind) families at reach 0 / "
      "1 / 7 / 64 / 400 (3 000 to 10 000 finite entries each), 4.0e-6 with a label outside the set leading by 320 … 640 inside the walks, "
      "1.3e-4 on the 2 000-item sequence whose starts 1 500 … 1 990 items away have log p from −585 down to −780; the joint from closed runs "
      "sums to `log_start` within 8.6e-8 of the bound; 50 anchors against 20 000 sampled paths: at most 1.2 σ.  The 70 cases take 13 s, the "
      "longest (the typed front end: a fit, five predictions and two command lines) 5.2 s.")
    A("* Not measured: how the pass, the host checks and the copies divide inside the call; reaches beyond the sequences' length; a batch "
      "with many more anchors than sequences (walks then share the device better); the typed front end's call.\n")
    print_wrapped(out)


def section_7n():
    """§7n from profiles/minrun_marginals_bench.jsonl and, for the max walk's neighbours, profiles/minrun_bench.jsonl (``python
    tools/measurements_md.py --section 7n``): appended to MEASUREMENTS.md behind §7m."""
    rows = [json.loads(ln) for ln in open(os.path.join(P, "minrun_marginals_bench.jsonl")) if ln.strip()]
    med = lambda t, name: t["kernel_us"][name]["median"]
    t0 = rows[0]
    out = []
    A = out.append
    A("### 7n. Marginals under a minimum run length: `gecco_crf_marginals_min_run` (`tools/bench_minrun.py --marginals`, "
      "`minrun_marginals_bench.jsonl`)\n")
    A(f"`Model.marginals_min_run` (DESIGN.md §4.9m) on §7l's batch: {t0['items']} items as {t0['sequences']} sequences of "
      f"{t0['items'] // t0['sequences']}; weights N(0, 0.5); the label set is every label but label 0; `marg` and `inside` both asked for.  "
      "No threshold was set: these are records.  Kernel times are begin-to-end durations from one `rocprofv3 --kernel-trace --stats` run "
      "of its own (`--trace-pass --marginals`: per label count and minimum one warm-up call and three traced calls of `viterbi_min_run` "
      "with log Z_C, then as many of `marginals_min_run`, nothing else); medians of the three, µs.  The sum-semiring launch of "
      "`viterbi_min_run` is the parent commit's code path (the same source with the store compiled out), in the same run.  The pass is "
      "the sum of the launches of a `marginals_min_run` call before its own two: the whole-contig forward-backward that every lattice "
      "query runs first (gl_state keeps the raw state scores; its marginals are not brought back).\n")
    A("| L | m | forward, sum, values kept | `gl_minrun_backward` | the two launches | `viterbi_min_run`'s forward, sum | two launches / "
      "that | kept forward / plain forward | the pass | forward values |")
    A("|---|---|---|---|---|---|---|---|---|---|")
    for t in rows:
        A(f"| {t['labels']} | {t['min_run']} | {med(t, 'gl_minrun_forward_sum_store'):.0f} | {med(t, 'gl_minrun_backward'):.0f} | "
          f"{t['two_launches_us']:.0f} | {med(t, 'gl_minrun_forward_sum'):.0f} | {t['two_launches_over_forward_sum']:.2f} | "
          f"{med(t, 'gl_minrun_forward_sum_store') / med(t, 'gl_minrun_forward_sum'):.2f} | {med(t, 'marginals_pass'):.0f} | "
          f"{t['forward_value_bytes'] / 1e6:.1f} MB |")
    A("")
    lo = min(t["two_launches_over_forward_sum"] for t in rows)
    hi = max(t["two_launches_over_forward_sum"] for t in rows)
    big = rows[-1]
    A("What the figures say, and what they do not:\n")
    A(f"* **The call's two launches take {lo:.1f} to {hi:.1f} times the sum-semiring launch that exists without it** -- at or below the two "
      "to three times that a second walk plus a stored and re-read workspace suggested.  The factor falls with the label count and the "
      "minimum: the forward body reads two slots of every source at d = m, the transposed table of the backward walk has no such state, "
      "so the backward launch is the cheaper of the two from m = 3 on.")
    A(f"* **Keeping the forward values costs {100 * (min(med(t, 'gl_minrun_forward_sum_store') / med(t, 'gl_minrun_forward_sum') for t in rows) - 1):.0f} to "
      f"{100 * (max(med(t, 'gl_minrun_forward_sum_store') / med(t, 'gl_minrun_forward_sum') for t in rows) - 1):.0f} %** of the forward launch; the workspace stream is "
      f"far from binding: at L = {big['labels']} and m = {big['min_run']} the forward launch writes {big['forward_value_bytes'] / 1e6:.0f} MB in "
      f"{med(big, 'gl_minrun_forward_sum_store') / 1e3:.1f} ms and the backward launch reads them in {med(big, 'gl_minrun_backward') / 1e3:.1f} ms, "
      f"{big['forward_value_bytes'] / med(big, 'gl_minrun_forward_sum_store') / 1e3:.0f} and {big['forward_value_bytes'] / med(big, 'gl_minrun_backward') / 1e3:.0f} GB/s.  "
      "Both walks are bound by the fp64 exponentials issued along a dependent walk (DESIGN.md §4.9m has the count), as §7l found for "
      "the max walk's instruction issue.")
    A("* The pass costs what it costs every lattice query and does not depend on the minimum.")
    A("* Accuracy, from `tests/test_gpu_minrun_marginals.py` on an MI355X (30 cases, 9 s; the longest, the typed front end with a fit, "
      "three predictions and three command lines, 5.5 s; the largest seam case, 8 labels at a minimum of 32, under a second): against the "
      "forward-backward over the explicit expanded state list in `numpy.longdouble`, over L = 2, 3, 5, 8, 32 and m = 1, 2, 3, 32, the "
      "fifteen seam lengths in one batch, three label sets and both weight families (N(0, 1), and N(0, 30) state scores with N(0, 10) "
      "transitions), **the largest relative error of a marginal / bound was 0.0115** (a seam case at L = 2 and m = 2; 0.0109 against "
      "enumeration's short sequences, 0.0023 with state scores of ±700 per item), the bound being expm1(3 (T + 1)(2 L + 8) ε max(1, M) + (m + 4) ε).  log Z_C was "
      "bit-equal to `viterbi_min_run`'s in every case, `inside` with `marg` NULL had the bytes it has with both, and every contig run "
      "alone had the bytes it has inside its batch.")
    A("* Not measured: the call as a whole (plan build, upload, the allocation of the workspace, the downloads: 8 bytes a gene for "
      "`inside`, 8 L more for `marg`), a minimum of 32 (the kernels' time grows about linearly in m, §7l), one long contig (the walks are "
      "sequential), other label sets, counters of the new kernels, and the typed front end's call.\n")
    A("Existing paths did not move.  The two instantiations of `gl_minrun_forward` that existed compile to the instruction streams they had "
      "(the ISA of the parent's file and of this one compared function by function), and calls without the new entry run the launches "
      "they ran: the whole GPU suite passes (2 178 cases with the 30 new ones, 280 s; 813 without a device).  `bench.py --gpus 1 --steps "
      "1000 --warmup 100 --no-cpu-baseline --no-latency --no-past-l3 --no-levels --no-8d --no-c4` (the 2-label flagship, whose kernels are "
      "untouched), the parent's tree and this one alternating on one box: parent 24.02, 24.13, 24.20 µs per step; change 24.02, 24.11, "
      "24.08.\n")
    print_wrapped(out)


def section_7o():
    """§7o from profiles/counts_bench.jsonl (``python tools/measurements_md.py --section 7o``): appended to MEASUREMENTS.md behind
    §7n."""
    rows = [json.loads(ln) for ln in open(os.path.join(P, "counts_bench.jsonl")) if ln.strip()]
    med = lambda t, name: t["kernel_us"][name]["median"]
    t0 = rows[0]
    out = []
    A = out.append
    A("### 7o. Run-count posteriors: `gecco_crf_run_counts` (`tools/bench_counts.py`, `counts_bench.jsonl`)\n")
    A(f"`Model.run_counts` (DESIGN.md §4.9n) on §7l's batch: {t0['items']} items as {t0['sequences']} sequences of "
      f"{t0['items'] // t0['sequences']}; weights N(0, 0.5); the label set is every label but label 0; `log_mass`, `score` and `y` all asked "
      "for.  No threshold was set: these are records, and nobody had measured this kernel before.  Kernel times are begin-to-end durations "
      "from one `rocprofv3 --kernel-trace --stats` run of its own (`--trace-pass`: per label count and K one warm-up call and three traced "
      "calls of `run_counts`, then as many of `viterbi_min_run` with log Z_C, nothing else); medians of the three, µs.  The comparison is "
      "`viterbi_min_run` at a minimum of K + 1, which gives its lanes the same K + 1 slots a gene -- except at K = 32, where K + 1 = 33 is "
      "beyond that entry's range and the minimum is 32: 33 slots against 32.\n")
    A("| L | K | slots | `gl_counts_forward`, sum | `gl_counts_forward`, max | `gl_counts_backtrack` | min-run m | `gl_minrun_forward`, sum | "
      "`gl_minrun_forward`, max | `gl_minrun_backtrack` | sum / min-run sum | max / min-run max | back-pointers |")
    A("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for t in rows:
        A(f"| {t['labels']} | {t['max_runs']} | {t['slots']} | {med(t, 'gl_counts_forward_sum'):.0f} | {med(t, 'gl_counts_forward_max'):.0f} | "
          f"{med(t, 'gl_counts_backtrack'):.0f} | {t['min_run']} | {med(t, 'gl_minrun_forward_sum'):.0f} | {med(t, 'gl_minrun_forward_max'):.0f} | "
          f"{med(t, 'gl_minrun_backtrack'):.0f} | {t['sum_over_min_run_sum']:.2f} | {t['max_over_min_run_max']:.2f} | "
          f"{t['back_pointer_bytes'] / 1e6:.1f} MB |")
    A("")
    ratios = [t[k] for t in rows for k in ("sum_over_min_run_sum", "max_over_min_run_max")]
    big = rows[-1]
    A("What the figures say, and what they do not:\n")
    A(f"* **The counts launches take {min(ratios):.2f} to {max(ratios):.2f} times their min-run siblings at equal slots** -- nowhere near the "
      "factor of two that would have called for a profile.  A counts destination reads one slot of every source label and a second one at "
      "the tail slot only, which is what a min-run destination does at d = m; the inside lanes' extra address select (one slot lower for an "
      "outside source) does not show.  Where the counts launch is the cheaper one (few slots, many labels) the min-run body presumably "
      "pays for its slot-dependent source masks; that was not looked into.")
    A("* **The time grows about linearly in the slot count**, as the min-run walks' does in m: the sum launch takes "
      f"{rows[0]['forward_sum_ns_per_item']:.1f} ns an item at L = {rows[0]['labels']}, K = {rows[0]['max_runs']} and "
      f"{big['forward_sum_ns_per_item']:.0f} ns at L = {big['labels']}, K = {big['max_runs']}.  The body is §7l's and §7n's: fp64 "
      "exponentials (sum) and compare-selects (max) issued along a dependent walk, one wave a workgroup, "
      f"{big['sequences'] * 32 // 64} waves at 32 labels; no profile beyond the trace was taken.  Skipping the slots that cannot be "
      "reached yet (c > ⌈(t + 1) / 2⌉) would save at most the first 2 K genes of a contig; it was not built.")
    A(f"* The backtrack, one lane per (sequence, k), takes {min(med(t, 'gl_counts_backtrack') for t in rows):.0f} to "
      f"{max(med(t, 'gl_counts_backtrack') for t in rows):.0f} µs: K + 1 times the lanes of the min-run backtrack, which keeps more of the "
      "device busy on a walk that is latency-bound either way.")
    A("* Accuracy, from `tests/test_gpu_counts.py` on an MI355X (58 cases, 32 s; the largest seam case, 32 labels at K = 32, 3.4 s): against the recursion over the explicit counter table in `numpy.longdouble`, over L = 2, 3, 4, 8, 9, 16, 17, 32 and K = 1, "
      "2, 3, 5, 16, 32, the thirteen seam lengths in one batch, four label sets and the four kinds of batch, **the largest |log Z_k error| / "
      "bound was 0.040**, the bound being (T + 1)(2 L + 8) ε max(1, M); −∞ exactly where the yardstick has −∞.  With integer weights every "
      "plane's labels were the yardstick's and every score bit-equal; the largest of a sequence's scores had the bits of "
      "`viterbi_kbest`'s rank 0 in both weight families; either output had the bytes it has when the other is not asked for.")
    A("* Not measured: the call as a whole (plan build, upload, the allocation of the back-pointers, the downloads: 16 (K + 1) bytes a "
      "sequence and K + 1 bytes a gene), one long contig (the walk is sequential), other label sets, counters of the new kernels, and "
      "the typed front end's calls.\n")
    A("Existing paths did not move: no shared kernel, launcher or plan path changed, and calls without the new entry run the launches "
      "they ran.  The whole GPU suite passes (2 236 cases with the 58 new ones and 1 skipped as before, 310 s; 839 without a device).  "
      "`bench.py --gpus 1 --steps 1000 --warmup 100 --no-cpu-baseline --no-latency --no-past-l3 --no-levels --no-8d --no-c4` (the 2-label "
      "flagship, whose kernels are untouched), the parent's tree and this one alternating on one box: parent 24.21, 24.28 µs per step; "
      "change 24.22, 24.28.\n")
    print_wrapped(out)


def section_walk():
    """The contig-walk refactor's section from profiles/walk_refactor_ab.txt and profiles/walk_bits.txt (``python
    tools/measurements_md.py --section walk``): appended to MEASUREMENTS.md behind the lattice refactor's."""
    ab = [ln.rstrip("\n") for ln in open(os.path.join(P, "walk_refactor_ab.txt"))]
    bits = [ln for ln in open(os.path.join(P, "walk_bits.txt")) if ln.strip()]
    kernels = [ln for ln in ab if " | parent " in ln and " | change " in ln]
    tally = [ln for ln in ab if ln.startswith("inside ")][-1]
    whole = [ln for ln in ab if ln.startswith("figures whose every run")][-1]
    cases = sum(int(ln.split(" | cases ")[1].split(" ")[0]) for ln in bits)
    out = []
    A = out.append
    A("## One contig-walk frame for the K-best, min-run and run-count kernels, parent commit against the change (`walk_refactor_ab.txt`, "
      "`walk_bits.txt`)\n")
    A("`crf_contig_walk.hpp` holds the frame of `gl_kbest_forward`, `gl_minrun_forward`, `gl_minrun_backward` and `gl_counts_forward` once "
      "(DESIGN.md §4.9i, k, m, n).  **Resources**: `walk_refactor_ab.txt` opens with the `-Rpass-analysis=kernel-resource-usage` table of "
      f"the {len(kernels)} kernels of the three files in both builds; {[ln for ln in ab if ln.startswith('conditions missed')][-1]} (no scratch "
      "anywhere, no kernel's occupancy below its parent's).  **Bits**: `tools/walk_bits.py` under `GECCO_CRF_LIBRARY` with the parent's library "
      f"and the change's in one job gave the same file, {cases} cases in {len(bits)} blocks (`walk_bits.txt` is the short form).  **Time**: "
      "`tools/bench_kbest.py`, `tools/bench_minrun.py`, `tools/bench_counts.py` at their defaults and `bench.py`, parent and change "
      f"alternating on one MI355X, three pairs, every run against the parent's own range: {tally}; {whole}.\n")
    print_wrapped(out)


def print_wrapped(out):
    import textwrap

    wrapped = []
    for block in "\n".join(out).split("\n"):
        if block.startswith(("|", "#")) or not block:
            wrapped.append(block)
        else:
            wrapped.append(textwrap.fill(block, width=125, subsequent_indent="  " if block.startswith("* ") else "", break_long_words=False,
                                         break_on_hyphens=False))
    print("\n".join(wrapped))


def main():
    import sys

    if sys.argv[1:] == ["--section", "7m"]:
        return section_7m()
    if sys.argv[1:] == ["--section", "7n"]:
        return section_7n()
    if sys.argv[1:] == ["--section", "7o"]:
        return section_7o()
    if sys.argv[1:] == ["--section", "walk"]:
        return section_walk()
    c3, c3d = J("bench_c3_detail"), J("bench_c3_driver_command_detail")
    line = open(os.path.join(P, f"{TAG}_bench_c3_driver_command.json")).read().strip()
    c1, c2, c5, two = J("bench_c1_detail"), J("bench_c2_detail"), J("bench_c5_detail"), J("bench_c3_two_launch_detail")
    pmc = J("pmc")
    summ = open(os.path.join(P, f"{TAG}_rocprofv3_summary.txt")).read()
    c5s = open(os.path.join(P, f"{TAG}_c5_rocprofv3_summary.txt")).read()
    lv, wc, lat = J("levels"), J("whole_contig"), c3["latency"]
    r = c3["roofline"]
    w = c3["roofline_window_kernel"]
    alg = r["algorithmic_bytes_per_launch"]
    step = us(c3["ms_per_step"])
    cpu1, cpun = c3["cpu_baseline"]["value"], c3["cpu_baseline_all_cores"]
    par = c3["parity"]
    kt_calls, kt_us = kt(summ, "kt/", "crf_decode_pipelined")
    kt2_calls, kt2_us = kt(summ, "kt2/", "crf_decode_pipelined")
    ktw_calls, ktw_us = kt(summ, "ktw/", "crf_windowed_l2")
    pp, pn = pmc["C3:pipelined"], pmc.get("C3:pipelined:no_handover_store", {})
    out = []
    A = out.append
    A("# Measurements, round 6\n")
    A("Generated by `tools/measurements_md.py` from the committed records: every figure is read from the file it names (`INDEX.md` says how each\n"
      "was produced).  One GPU run of `tools/r6_profiles.sh` (removed; see git history) on one MI355X box produced the `r06_*` set (kernel source hash\n"
      f"`{pp.get('kernel_source_sha16')}`); boxes of the pool differ by ±3 %, the host-bound figures (launch-bound steps, API levels) by more.  The round-5\n"
      "kernel descriptions with their numbers are kept verbatim in `MEASUREMENTS_r05.md`; the kernels on the headline path did not change\n"
      "this round (the launch's argument block and the host side of a call did).\n")
    A("## 1. The headline: one MI355X, C3 (BASELINE.json `configs[2]`: 10 000 contigs, 1 999 989 genes, SURVEY §8d's law)\n")
    A("| | value | file |\n|---|---|---|")
    A(f"| step (windowed marginals + Viterbi labels of one resident batch, pipelined over two decode streams), default run | **{step:.1f} µs = "
      f"{c3['value'] / 1e9:.1f} G genes/s** | `r06_bench_c3.json` |")
    A(f"| the driver's own command (`--gpus 1 --steps 20 --warmup 5`: every 20-step region pays its pipeline fill and flush) | "
      f"{us(c3d['ms_per_step']):.1f} µs = {c3d['value'] / 1e9:.1f} G genes/s | `r06_bench_c3_driver_command.json` ({len(line.encode())} bytes; round 5's line was "
      "29 KB and could not be parsed) |")
    A(f"| one decode stream / two plain launches per batch | {us(c3['one_stream_ms_per_step']):.1f} / {us(c3['two_launch_ms_per_step']):.1f} µs "
      f"(`--schedule two-launch` run: {us(two['ms_per_step']):.1f}) | `r06_bench_c3_detail.json`, `r06_bench_c3_two_launch.json` |")
    A(f"| CPU port (C oracle driven window by window like the reference), 1 thread / {cpun['cores']} threads | {cpu1 / 1e6:.2f} M / "
      f"{cpun['value'] / 1e6:.1f} M genes/s ({sci(c3['value'] / cpu1)}× / {sci(c3['value'] / cpun['value'])}× below the step) | same |")
    A(f"| parity of the whole batch against the oracle | max \\|Δp\\| {par['max_abs_dp_vs_oracle']:.1e}, {par['cluster_call_mismatches']} cluster-call "
      f"mismatches, {par['viterbi_label_mismatches']} label mismatches of {par['genes_checked']} | same |")
    A("")
    A(f"**The roofline record** (`roofline` in the line; dominant kernel `{r['kernel']}`):\n")
    A("| field | value | how |\n|---|---|---|")
    A(f"| `algorithmic_bytes_per_launch` | {alg} | 4(n+1) + 4·nnz + 8n + 4(nc+1) + n (DESIGN §3) |")
    A(f"| `kernel_us` (live, HIP events, back-to-back launches on ONE stream; pre-rolled, median of three series) | {r['kernel_us']:.2f} "
      f"(the 20-step run: {c3d['roofline']['kernel_us']:.2f}) | `r06_bench_c3_detail.json` |")
    A(f"| `kernel_us_rocprof` (committed `rocprofv3 --kernel-trace --stats` of `bench.py --streams 1`, {kt_calls} launches) | {kt_us:.3f} | "
      "`r06_rocprofv3_summary.txt` (`kt`), `pmc_traffic.json` |")
    A(f"| `frac` / `frac_rocprof` (of 8 TB/s) | **{r['frac']:.4f} / {r['frac_rocprof']:.4f}** | {alg} B ÷ µs ÷ 8 TB/s; events and trace "
      f"differ by {abs(r['kernel_us'] / kt_us - 1) * 100:.1f} % |")
    A(f"| `kernel_us_isolated` (one launch on an idle device between two events) / `kernel_us_in_flight` (two decode streams: two launches "
      f"overlap) | {r['kernel_us_isolated']:.1f} / {r['kernel_us_in_flight']:.1f} (rocprof `kt2`: {kt2_us:.1f}) | a launch in flight lasts longer, a "
      f"batch leaves every {step:.0f} µs: `frac_of_step` {r['frac_of_step']:.3f} |")
    A(f"| `traffic` (FETCH_SIZE × 2 + WRITE_SIZE, separate `--pmc` passes) | {pp['hbm_bytes_per_launch']} B = {pp['hbm_bytes_per_launch'] / alg:.2f}× "
      f"algorithmic | `r06_pmc.json`: FETCH {pp['FETCH_SIZE_KB']:.0f} KB, WRITE {pp['WRITE_SIZE_KB']:.0f} KB |")
    A(f"| `limiter` | fp64 VALU issue: {pp['SQ_INSTS_VALU'] / 1e6:.2f} M wave instructions × 4 cycles / ({r['kernel_us']:.2f} µs × 1 024 SIMDs × "
      f"2.4 GHz) = **{r['valu_frac']:.2f}**; at the step rate {r['valu_frac_of_step']:.2f}, at the rate the chip sustains on fp64 (4.7 cycles, "
      f"`tools/ubench/valu_rates.hip`) {r['valu_frac_of_step_at_sustained_rate']:.2f} | `r06_pmc.json` |")
    A("")
    A(f"**Window kernel alone** (`roofline_window_kernel`): {w['kernel_us']:.1f} µs by events = {w['frac']:.3f} of 8 TB/s; {ktw_us:.2f} µs in the "
      f"`--windowed-only` trace (`ktw`, {ktw_calls} launches) = {w['frac_rocprof']:.3f}; counter traffic {pmc['C3']['hbm_bytes_per_launch'] / 1e6:.1f} MB for "
      f"{w['algorithmic_bytes_per_launch'] / 1e6:.1f} MB; past the Infinity Cache (2·10⁸ genes) {c3['roofline_past_l3']['frac']:.3f}; under the `genome` "
      f"weight law {c3['roofline_genome']['frac']:.3f} (step {us(c3['roofline_genome']['ms_per_step']):.1f} µs).  **Why rounds 4–5 (and this round's first "
      "set) show 29.3–29.5 µs for it in the kernel trace against 25.5–26 µs by events**: the symbol `crf_windowed_l2<20, true, false, 256, 2>` "
      "also serves the FIRST launch of the two-launch schedule, which writes the score differences too (~31.6 µs); the trace of a bench "
      "run held 203 plain launches and 270 of those: (203 × 26.1 + 270 × 31.6) / 473 = 29.2.  `tools/profile.sh` now takes a trace with "
      "`--windowed-only` for this kernel, and the pre-roll loops add plain launches to the other traces.  What remains between events and "
      "trace is the difference between the interval at which back-to-back launches complete and a launch's own begin-to-end time, plus the "
      "trace's overhead.  The driver's `--steps 20` run used to report `kernel_us` 33.7 (device not at its clocks after short regions with a "
      "wait each): the kernel timings are now pre-rolled and the median of three series.\n")
    A("## 2. The other configurations\n")
    A("| configuration | step | file |\n|---|---|---|")
    l50 = {k: v["median_us"] for k, v in lat["50"].items() if isinstance(v, dict) and "median_us" in v}
    floor = lat.get("launch_floor_us", {})
    A(f"| C1 (`configs[0]`: one 50-gene contig, pretrained weights), resident step | {us(c1['ms_per_step']):.2f} µs (host issue "
      f"{c1['host_issue_us_per_step']:.1f} µs per launch) | `r06_bench_c1_detail.json` |")
    A(f"| C1, host to host: `gecco_crf_windowed_marginals` / decode on the compact wire / cluster rows / `predict_probabilities` on objects | "
      f"{l50['one_shot_pinned']:.1f} / {l50['decode_wire']:.1f} / {l50['clusters_wire']:.1f} / {l50['object_api']:.0f} µs | `latency` in "
      "`r06_bench_c3_detail.json`, `r06_latency.json` |")
    A(f"| C2 (`configs[1]`: 1 000 contigs, 0.2 M genes) | **{us(c2['ms_per_step']):.2f} µs = {c2['value'] / 1e9:.0f} G genes/s** (round 5: 5.4–6.3; host issue "
      f"{c2['host_issue_us_per_step']:.1f} µs per launch) | `r06_bench_c2_detail.json` |")
    sh, shd = c3["c4_shard"], c3d["c4_shard"]
    A(f"| 8-way shard of C3 (`configs[3]`, {sh['genes']} genes) on one device | {us(sh['c4_shard_ms']):.1f} µs in the default run, "
      f"{us(shd['c4_shard_ms']):.1f} in the 20-step run (round 5: 5.7–7.4; host issue {sh['host_issue_us_per_step']:.1f} µs) | `c4_shard` in "
      "`r06_bench_c3_detail.json` |")
    ch = {k: kt(c5s, "kt_results.db", k)[1] for k in ("vd_fold", "vd_replay", "v_labels_refine", "vd_exact_fix")}
    A(f"| C5 (`configs[4]`: 100 × 50 000 genes) | **{us(c5['ms_per_step']):.1f} µs = {c5['value'] / 1e9:.1f} G genes/s** (window kernel alone "
      f"{c5['roofline']['kernel_us']:.1f} µs = {c5['roofline']['frac']:.3f} of 8 TB/s; `vd_fold` {ch['vd_fold']:.1f} + `vd_replay` {ch['vd_replay']:.1f} + "
      f"`v_labels_refine` {ch['v_labels_refine']:.1f} + `vd_exact_fix` {ch['vd_exact_fix']:.1f} µs under contention) | `r06_bench_c5_detail.json`, "
      "`r06_c5_rocprofv3_summary.txt` |")
    for name in ("C3", "C5"):
        v = wc[name]
        A(f"| rows F / V stand-alone, {name}: whole-contig marginals with log Z / without, Viterbi labels only / with scores | "
          f"{us(v['marginals_full']['ms']):.1f} / {us(v['marginals_full_without_log_z']['ms']):.1f} / {us(v['viterbi_labels_only']['ms']):.1f} / "
          f"{us(v['viterbi_with_scores']['ms']):.1f} µs | `r06_whole_contig.json` |")
    A("| any-L kernels (L = 3 … 32) | unchanged from round 5 | `r06_general_l.json`, `r06_general_levels_rocprofv3_summary.txt` |")
    A("")
    A("**Small batches are bound by the host's launch path, not by the GPU** (`r06_ab_raw.txt`: `tools/host_issue_probe.py`, `tools/r6_streams.sh` (removed; see git history)): "
      "one `gecco_crf_plan_run_decode_pipelined` call costs the host 3.4–4.9 µs whatever the batch (2 011 or 200 054 genes), a plain windowed "
      "launch 3.4–4.5, against 2.9 µs for an EMPTY kernel launched from C and 3.6–3.8 with a 400-byte argument (`r06_launch_floor_pcie.txt`); with "
      "two or more decode streams the step of such a batch IS that issue time.  Round 5 spent 4.7–5.5 µs per call: the model constants of the "
      "argument blocks are now computed once per device (17 `exp`, 36 divisions, 3 `getenv` per call before), the device is switched only when "
      "the thread is on another one, the launch carries a compact 624-byte block (1 128 before), and `Plan.bind_decode_pipelined` converts the "
      f"Python arguments once.  A step of the 8-way shard therefore strong-scales to ≈ {step:.0f} / {us(sh['c4_shard_ms']):.1f} = "
      f"{step / us(sh['c4_shard_ms']):.1f}× of 8 even on perfect hardware — what `configs[3]` will show on a node is the launch path of eight processes.\n")
    A("## 3. Through the API levels (C3 unless said; `levels` in `r06_bench_c3_detail.json`, `r06_levels.json`)\n")
    L = c3["levels"]
    bl = lv["batch_driver_levels"]
    A("| level | time | rate |\n|---|---|---|")
    A(f"| resident step | {c3['ms_per_step']:.3f} ms | {c3['value'] / 1e9:.1f} G genes/s |")
    A(f"| host buffers, pinned, one-shot C ABI (H2D + kernels + D2H) | {bl['one_shot_pinned']['ms']:.2f} ms ({bl['one_shot_pinned_degree_bytes']['ms']:.2f} with degree "
      f"bytes; pageable {bl['one_shot_pageable']['ms']:.2f}) | {bl['one_shot_pinned']['genes_per_s'] / 1e9:.1f} G genes/s — the PCIe-inclusive rate; never `value` |")
    A(f"| marginals + labels, compact wire | {bl['decode_pinned_wire16']['ms']:.2f} ms | {bl['decode_pinned_wire16']['genes_per_s'] / 1e9:.1f} G |")
    A(f"| cluster rows only, compact wire | {bl['cluster_rows_wire16_pinned']['ms']:.2f} ms | {bl['cluster_rows_wire16_pinned']['genes_per_s'] / 1e9:.1f} G |")
    t = lv["columnar_tables_api"]
    A(f"| table columns in → table columns out (`predict_tables`, {t['genes'] / 1e6:.1f} M genes / {t['domain_rows'] / 1e6:.1f} M rows) | {t['ms']:.1f} ms "
      f"({L['predict_tables']['ms']:.1f} ms per {L['predict_tables']['genes'] / 1e6:.1f} M in the bench record) | **{t['genes_per_s'] / 1e6:.0f} M genes/s** (round 5: 30 M; "
      "the output columns' gather and order checks are native multi-threaded passes now) |")
    o = lv["python_object_api"]
    A(f"| `Gene` objects in → `Gene` objects out | {o['ms']:.0f} ms per {o['genes'] // 1000} k genes ({L['object_api']['ms']:.0f} ms per "
      f"{L['object_api']['genes'] // 1000} k in the bench record) | {o['genes_per_s'] / 1e6:.2f}–{L['object_api']['genes_per_s'] / 1e6:.2f} M genes/s |")
    cli = lv["columnar_cli_tsv_to_tsv"]
    A(f"| TSV → TSV (`python -m gecco_amd.predict`) | {cli['ms']:.0f} ms per {cli['genes'] / 1e6:.1f} M genes | {cli['genes_per_s'] / 1e6:.1f} M genes/s |")
    smd = c3["session_multi_device"]
    A(f"| a session over eight entries of device 0 (the multi-device machinery on one device) | {smd['eight_entries_of_device_0']['ms']:.2f} ms vs "
      f"{smd['one_device']['ms']:.2f} | `session_multi_device` |")
    A("")
    A("## 4. Reference-bits mode (`r06_reference_bits.jsonl`, `r06_ab_raw.txt`, `parity` in the bench record)\n")
    rb, fk, rc = par["reference_bits_vs_libm_oracle"], par["fast_kernels_vs_libm_oracle"], par["reference_bits_vs_correctly_rounded_oracle"]
    rbl = [json.loads(x) for x in open(os.path.join(P, f"{TAG}_reference_bits.jsonl")) if x.strip()]
    res = {d["mode"]: d for d in rbl if "mode" in d}
    one = next(d for d in rbl if "one_shot_pinned_ms" in d)["one_shot_pinned_ms"]
    c1s = next(d for d in rbl if "c1_one_shot_us" in d)["c1_one_shot_us"]
    gt = par["golden_tables"]
    nf = sum(gt[k]["float_cells"] for k in ("genes", "features", "clusters"))
    nfd = sum(gt[k]["float_cells_differing"] for k in ("genes", "features", "clusters"))
    nfr = sum(gt["reference_bits_mode"][k]["float_cells_differing"] for k in ("genes", "features", "clusters"))
    nx = sum(gt[k]["exact_cells"] for k in ("genes", "features", "clusters"))
    nxd = sum(gt[k]["exact_cells_differing"] for k in ("genes", "features", "clusters"))
    A(f"C3, {rb['genes']} genes: **bit-identical to the oracle run with a correctly rounded `exp` on every gene ({rc['genes_differing']} differ); against the "
      f"oracle run with the box's glibc `exp` — what CRFsuite calls — {rb['genes_differing']} genes ({rb['genes_differing'] / rb['genes'] * 100:.2f} %) differ, by at "
      f"most {rb['max_ulps']} ulps** (exactly the genes on which the two oracles differ); the fast kernels differ from the libm oracle on "
      f"{fk['genes_differing']} genes ({fk['genes_differing'] / fk['genes'] * 100:.0f} %), by at most {fk['max_ulps']} ulps (max |Δp| {par['max_abs_dp_vs_oracle']:.1e}).  "
      f"{par['cluster_call_mismatches']} cluster-call mismatches in either mode.  Cost: {res['reference bits']['resident_windowed_ms']:.3f} ms per resident C3 batch = "
      f"{res['reference bits']['genes_per_s'] / 1e9:.1f} G genes/s ({res['reference bits']['resident_windowed_ms'] / res['fast kernels']['resident_windowed_ms']:.1f}× the fast "
      f"window kernel), one-shot pinned {min(one['reference_bits']):.2f} vs {min(one['fast']):.2f} ms, one 50-gene contig {min(c1s['reference_bits']):.1f} vs "
      f"{min(c1s['fast']):.1f} µs; the table and object levels do not notice the mode.  The reference's fixture files: {nf - nfr} of {nf} float cells "
      f"string-identical in this mode, {nf - nfd} of {nf} from the fast kernels (≤ {max(gt[k]['max_ulps'] for k in ('genes', 'features', 'clusters'))} ulps away), "
      f"{nx - nxd} of {nx} text / integer cells in both (`parity.golden_tables`).\n")
    A("## 5. The hand-over between launches, bounded by counters (`r06_rocprofv3_summary.txt`, `r06_pmc.json`, `r06_ab_raw.txt`)\n")
    if pn:
        A(f"With the hand-over's stores switched off (a round-6 A/B switch of the library, since retired; the tiles keep their score differences; labels wrong): WRITE_SIZE {pp['WRITE_SIZE_KB']:.0f} → "
          f"{pn['WRITE_SIZE_KB']:.0f} KB, FETCH_SIZE {pp['FETCH_SIZE_KB']:.0f} → {pn['FETCH_SIZE_KB']:.0f} KB, traffic {pp['hbm_bytes_per_launch'] / 1e6:.1f} → "
          f"{pn['hbm_bytes_per_launch'] / 1e6:.1f} MB ({pp['hbm_bytes_per_launch'] / alg:.2f}× → {pn['hbm_bytes_per_launch'] / alg:.2f}×), `SQ_INSTS_VALU` "
          f"{pp['SQ_INSTS_VALU'] / 1e6:.2f} → {pn['SQ_INSTS_VALU'] / 1e6:.2f} M; the step is 7–8 % shorter (`EXPERIMENTS.md`, round 6, item 6).\n")
    A("## 6. Multi-GPU (`r06_bench_2ranks_one_device.json`, `r06_bench_world1_nccl.json`)\n")
    r2, w1 = J("bench_2ranks_one_device"), J("bench_world1_nccl")
    A(f"No multi-GPU node was available: two gloo ranks on ONE device (a dry run of the N > 1 code path: weak line {us(r2['ms_per_step']):.1f} µs per step "
      f"for two batches, strong line {us(r2['strong_scaling']['ms_per_step']):.1f} µs for the halves) and RCCL at world size 1 "
      f"({us(w1['ms_per_step']):.1f} µs).  Not scaling measurements.")
    train_path = os.path.join(P, "train_bench.jsonl")
    if os.path.exists(train_path):
        A("\n## 7. Training: `gecco_crf_trainer_eval` and a whole fit (`train_bench.jsonl`, `tools/bench_train.py`)\n")
        A("Synthetic labelled set (`synth.synth_training_set`), every (attribute, label) pair and transition a feature, c1 = c2 = 0.15 (OWL-QN), "
          "libLBFGS's defaults.  An evaluation is the weights up, six launches, f and g down, synchronous (median of the timed calls).  "
          "Bytes: what the kernel layout has to move at least; the CPU yardstick is a single-thread numpy port of the same objective on a "
          "prefix of the set, scaled by window count (not CRFsuite, which is not available).\n")
        A("| W | items | windows | µs / eval | window positions / s | min bytes / eval | HBM share | fit: iterations / evals / wall | numpy port, scaled | speed-up |")
        A("|---|---|---|---|---|---|---|---|---|---|")
        for ln in open(train_path):
            t = json.loads(ln)
            f, cb = t["fit"], t["cpu_baseline"]
            A(f"| {t['window']} | {t['items']} | {t['windows']} | {t['eval_us']:.0f} | {t['window_positions_per_s'] / 1e9:.2f} G | "
              f"{t['min_bytes_per_eval'] / 1e6:.0f} MB | {100 * t['hbm_frac']:.1f} % | {f['iterations']} / {f['evaluations']} / {f['wall_s']:.2f} s "
              f"({f['status']}) | {cb['eval_s_scaled_to_set']:.2f} s | {cb['speedup_vs_device']:.0f}× |")
    ab_path = os.path.join(P, "train_bench_ab.jsonl")
    if os.path.exists(ab_path):
        A("\nThe window kernel's range check and log-space recomputation of flagged windows (`train_bench_ab.jsonl`): the parent "
          "build's library and this one, alternating on one box, two runs each, `--evals 50`.  At these weights no window is "
          "flagged, so the difference is the per-step check alone.\n")
        A("| W | build | run | µs / eval (median) | µs / eval (min) |")
        A("|---|---|---|---|---|")
        rows = [json.loads(ln) for ln in open(ab_path)]
        for t in sorted(rows, key=lambda t: (-t["window"], t["build"] != "parent", t["run"])):
            A(f"| {t['window']} | {t['build']} | {t['run']} | {t['eval_us']:.0f} | {t['eval_us_min']:.0f} |")
    print("\n".join(out))


if __name__ == "__main__":
    main()
