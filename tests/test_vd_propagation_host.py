"""The Viterbi workgroups' entering values by value propagation, on the host: a numpy model of fold + propagation +
fallback decision (tests/vd_propagation_model.py restates vd_short_block) against the strictly sequential difference
recursion -- whose labels are pinned to oracle_viterbi_delta's here.

Where a lane's left neighbour holds a constant map the value entering the lane must be the sequential recursion's bit
for bit; behind a run of other lanes it must lie within the workgroup's coarse margin (4 n + 4) ulp(M) of it, which is
what the kernel's "a lane whose decisions keep their distance has the sequential decisions already" rests on.  For
every planted batch the model also says whether the workgroup has to take the fallback (the scan of whole maps): the
GPU tests (tests/test_gpu_vd_propagation.py) rely on these answers."""
import numpy as np
import pytest

from tests import vd_propagation_model as vm


def _check(d, cptr, trans, wmax):
    from oracle import crf_oracle as orc

    w, _, gptr, attr = vm.batch_from_d(d, np.diff(cptr))
    delta = vm.sequential_delta(d, cptr, trans)
    assert np.array_equal(vm.labels_from_delta(delta, cptr, trans), orc.viterbi_delta(w, trans, cptr, gptr, attr))
    blocks = vm.run_model(d, cptr, trans)
    tmax = float(np.abs(trans).max())
    worst = 0.0
    for b in blocks:
        if b["fallback"]:
            continue
        margin = vm.coarse_margin(b["n"], wmax, tmax)
        for i in range(1, vm.LANES):
            if np.isnan(b["seq_in"][i]):
                continue
            got, want = float(b["din"][i]), float(b["seq_in"][i])
            if b["constant"][i - 1]:
                assert got == want, (b["g0"], i, got, want)
            else:
                worst = max(worst, abs(got - want) / margin)
                assert abs(got - want) <= margin, (b["g0"], i, got, want, margin)
    return blocks, worst


@pytest.mark.parametrize("law", ["8d", "genome"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_random_batches(law, seed):
    """metagenome-shaped batches under both weight laws of the bench model: no workgroup needs the fallback"""
    from gecco_amd import synth
    from oracle import crf_oracle as orc

    rng = np.random.default_rng(seed)
    A = 35000
    # the bench workloads' model (synth.workload), fresh contigs.  (How many lanes hold a constant map is a property of the
    # model: other draws of the same laws leave 13 % to 52 % of the lanes without one, and workgroups of the latter take the
    # fallback more often than not.  The values must be right either way -- that is asserted on every workgroup that
    # propagates -- but "no fallback" is asserted for this model only.)
    w, trans = synth.synth_model(A, np.random.default_rng(synth.SEED), law=law)
    lengths = synth.contig_lengths(rng, 120)
    cptr, gptr, attr = synth.synth_contigs(rng, lengths, A)
    st = orc.state_scores(w, gptr, attr)
    d = st[:, 1] - st[:, 0]
    # (the model's genes carry one attribute each; the margin's bound M only grows with more of them)
    blocks, worst = _check(d, cptr, trans, float(np.abs(w).max()))
    assert len(blocks) >= 10 and not any(b["fallback"] for b in blocks)
    nonconst = np.mean([np.mean(~b["constant"]) for b in blocks])
    assert 0.01 < nonconst < 0.5, nonconst
    print(f"law {law}: {len(blocks)} workgroups, {100 * nonconst:.1f} % of the lanes not constant, worst error / margin {worst:.2e}")


@pytest.mark.parametrize("law", ["8d", "genome"])
@pytest.mark.parametrize("seed", [1, 2])
def test_other_model_draws(law, seed):
    """other draws of the two weight laws: some workgroups take the fallback, the others' values are right"""
    from gecco_amd import synth
    from oracle import crf_oracle as orc

    rng = np.random.default_rng(seed)
    A = 3000
    w, trans = synth.synth_model(A, rng, law=law)
    cptr, gptr, attr = synth.synth_contigs(rng, synth.contig_lengths(rng, 120), A)
    st = orc.state_scores(w, gptr, attr)
    blocks, worst = _check(st[:, 1] - st[:, 0], cptr, trans, float(np.abs(w).max()))
    n_fb = sum(b["fallback"] for b in blocks)
    assert 0 < n_fb < len(blocks)
    print(f"law {law}, seed {seed}: {n_fb} of {len(blocks)} workgroups take the fallback, worst error / margin {worst:.2e}")


def test_weights_without_constant_lanes_take_the_fallback():
    """N(0, 1) weights (the tie planter's): most lanes' maps are not constant, runs exceed the bound"""
    rng = np.random.default_rng(5)
    lengths = [9, 200, 1, 2048, 3, 17] + [200] * 12
    d = rng.normal(0.0, 1.4, size=sum(lengths))
    cptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    blocks, _ = _check(d, cptr, vm.TRANS2, 1.4 * 6)
    assert any(b["fallback"] for b in blocks)


RUN_CASES = []
for _m in range(1, 9):
    for _at in (1, 64 - _m + 1, 64, 128 - _m // 2, 192 - _m + 1 if _m > 1 else 191):
        RUN_CASES.append((_at, _m))


@pytest.mark.parametrize("first_lane,lanes", RUN_CASES)
def test_planted_runs(first_lane, lanes):
    """runs of 1 .. 8 lanes at lane 1 and across the wave boundaries: exact behind constant lanes, inside the margin
    behind a run, and the fallback exactly when the part of a run that lies in ONE wave is longer than the bound (a run
    that straddles a wave boundary is worked off from both sides of the barrier: 6 + 2 lanes need no fallback, 7 do)"""
    rng = np.random.default_rng(100 * first_lane + lanes)
    n = 2048 - 5
    d = vm.plant_runs(rng, [(first_lane, lanes)], [n])
    cptr = np.array([0, n], dtype=np.int32)
    blocks, _ = _check(d, cptr, vm.TRANS2, 40.0)
    (b,) = blocks
    assert list(np.nonzero(~b["constant"])[0]) == list(range(first_lane, first_lane + lanes))
    assert b["fallback"] == vm.needs_fallback([(first_lane, lanes)])


def test_run_to_the_last_lane_with_genes():
    rng = np.random.default_rng(9)
    for n, lanes in ((8 * 200 + 3, 4), (2048, 3), (8 * 130, 6), (8 * 130 + 1, 7)):
        last = (n - 1) // 8
        d = vm.plant_runs(rng, [(last - lanes + 1, lanes)], [n])
        (b,), _ = _check(d, np.array([0, n], dtype=np.int32), vm.TRANS2, 40.0)
        # (a last lane that is partly padding is constant: padding positions are contig starts)
        want = list(range(last - lanes + 1, last + (1 if n % 8 == 0 else 0)))
        assert list(np.nonzero(~b["constant"])[0]) == want
        assert b["fallback"] == (len(want) > vm.RUN)


@pytest.mark.parametrize("waves", [(1,), (1, 2, 3)])
def test_waves_without_a_constant_lane(waves):
    """ONE contig of ~2000 genes: lane 0 holds the contig start, the named waves hold no constant lane -> fallback"""
    rng = np.random.default_rng(31 + len(waves))
    n = 2000
    d = vm.lane_background(rng, n)
    for w in waves:
        d[512 * w:min(512 * (w + 1), n)] = vm.quiet(rng, min(512 * (w + 1), n) - 512 * w)
    (b,), _ = _check(d, np.array([0, n], dtype=np.int32), vm.TRANS2, 40.0)
    for w in waves:
        genes_end = min(64 * (w + 1), n // 8)
        assert not b["constant"][64 * w:genes_end].any()
    assert b["constant"][0] and b["fallback"]


@pytest.mark.parametrize("pos", range(8))
def test_contig_boundaries_inside_a_lane_next_to_a_run(pos):
    """a contig ends / the next starts at position `pos` of the lane in front of a run, of its first lane and of the lane
    behind it: a lane that holds a contig start is constant"""
    rng = np.random.default_rng(50 + pos)
    for lane in (69, 70, 74):  # run: lanes 70 .. 73
        cut = 8 * lane + pos
        n = 1900
        lengths = [cut, n - cut]
        d = vm.lane_background(rng, n)
        d[8 * 70:8 * 74] = vm.quiet(rng, 32)
        # (the background's large first gene of a lane, where it now follows a contig start, is an ordinary gene again)
        cptr = np.array([0, cut, n], dtype=np.int32)
        (b,), _ = _check(d, cptr, vm.TRANS2, 40.0)
        assert b["constant"][lane] and not b["fallback"]
        inside = [i for i in range(70, 74) if i != lane]
        assert not b["constant"][inside].any()
