"""The Viterbi workgroups' value propagation on the device (crf_vd_short.hpp): labels equal to oracle.viterbi exactly, through
the kernel vd_short (Model.viterbi / Plan.run_viterbi without a score) and through the pipelined decode call, on batches
planted for the new pass and for its fallback.

Every case is one workgroup (a contig, or two, of about 2000 genes: whole contigs are packed into workgroups of at most 2048
genes, so consecutive cases never share one).  The host model (tests/vd_propagation_model.py, checked against the sequential
recursion in tests/test_vd_propagation_host.py) says for every workgroup whether it has to take the fallback -- the scan of
whole maps -- and the tests assert that answer against the cases' geometry before they look at the device:
  (a) runs of 1 .. 8 lanes whose maps are not constant, at lane 1, across the wave boundaries (lanes 63/64, 127/128, 191/192),
      at a wave's first lane, and ending on the workgroup's last lane with genes: the fallback exactly where the part of a run
      inside one wave is longer than the loop bound (6);
  (b) whole waves without one constant lane (wave 1; waves 1, 2 and 3 of a 2000-gene contig): the fallback;
  (c) contig ends / starts at every position 0 .. 7 of the lanes around a run: no fallback;
  (d) CRFsuite ties of 0 / +-1 / +-2 ulps (tests/helpers.py's construction) inside a run and at the first gene behind one,
      with the exact pass on (the default): no fallback, and every contig with a tie is decoded again."""
import functools

import numpy as np
import pytest

from tests import vd_propagation_model as vm

pytestmark = pytest.mark.gpu

N = 2048 - 5


@pytest.fixture(scope="module")
def nat():
    from gecco_amd import _native

    assert _native.device_count() >= 1
    return _native


def _assemble(cases):
    """cases: [(d, lengths, expected fallback)] -> one batch; every case lands in a workgroup of its own"""
    d = np.concatenate([c[0] for c in cases])
    lengths = [x for c in cases for x in c[1]]
    w, cptr, gptr, attr = vm.batch_from_d(d, lengths)
    cblk = vm.pack_blocks(cptr)
    starts = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])])
    assert cblk == [int(x) for x in starts], "a case shares a workgroup with its neighbour"
    return dict(d=d, w=w, cptr=cptr, gptr=gptr, attr=attr, expect=[c[2] for c in cases], n=int(cptr[-1]), ties=[])


def _finish(b):
    from oracle import crf_oracle as orc

    blocks = vm.run_model(b["d"], b["cptr"], vm.TRANS2)
    got = [blk["fallback"] for blk in blocks]
    assert got == b["expect"], [i for i, (x, y) in enumerate(zip(got, b["expect"])) if x != y]
    b["blocks"] = blocks
    b["ey"], _ = orc.viterbi(b["w"], vm.TRANS2, b["cptr"], b["gptr"], b["attr"])
    for g, winner in b["ties"]:
        assert b["ey"][g] == winner
    return b


@functools.lru_cache(maxsize=None)
def _batch(kind):
    rng = np.random.default_rng({"runs": 11, "waves": 12, "cuts": 13, "ties": 14}[kind])
    cases = []
    if kind == "runs":
        for m in range(1, 9):
            for at in (1, 64 - m + 1, 64, 128 - m // 2, 192 - m + 1 if m > 1 else 191, 127):
                cases.append((vm.plant_runs(rng, [(at, m)], [N]), [N], vm.needs_fallback([(at, m)])))
            # ... ending on the workgroup's last lane with genes (a full one; a partly padded lane is constant)
            n = 8 * 250
            cases.append((vm.plant_runs(rng, [(250 - m, m)], [n]), [n], vm.needs_fallback([(250 - m, m)])))
        # several runs in one workgroup, a lane apart
        runs = [(3, 2), (6, 6), (13, 1), (60, 4), (65, 3), (120, 6), (127, 6), (134, 5), (186, 6), (192, 6), (199, 1)]
        cases.append((vm.plant_runs(rng, runs, [N]), [N], False))
    elif kind == "waves":
        for waves in ((1,), (1, 2, 3), (2,), (3,)):
            n = 2000
            d = vm.lane_background(rng, n)
            for w in waves:
                d[512 * w:min(512 * (w + 1), n)] = vm.quiet(rng, min(512 * (w + 1), n) - 512 * w)
            cases.append((d, [n], True))
        cases.append((vm.quiet(rng, 2000), [2000], True))  # Delta inside (lo, hi) from the first gene to the last
    elif kind == "cuts":
        for pos in range(8):
            for lane in (69, 70, 72, 73, 74):  # run: lanes 70 .. 73
                n, cut = 1900, 8 * lane + pos
                d = vm.lane_background(rng, n)
                d[8 * 70:8 * 74] = vm.quiet(rng, 32)
                cases.append((d, [cut, n - cut], False))
    b = None
    if kind == "ties":
        ties = []
        for i, ulps in enumerate((0, 1, -1, 2, -2, 0, 1, -1)):
            run_at, m = (40, 3) if i % 2 == 0 else (62, 5)  # (the second run straddles lanes 63 / 64)
            d = vm.plant_runs(rng, [(run_at, m)], [N])
            # inside the run: genes 6 and 7 of its second lane; behind it: the first two genes of the lane that follows
            g = 8 * (run_at + 1) + 6 if i < 4 else 8 * (run_at + m)
            cases.append((d, [N], False))
            ties.append((i, g, ulps, i % 2))
        b = _assemble(cases)
        for i, g, ulps, j in ties:
            gg = i * N + g
            row0, row1, winner = vm.plant_tie(b["d"], b["cptr"], vm.TRANS2, gg, ulps, j)
            b["w"][gg], b["w"][gg + 1] = row0, row1
            b["d"][gg], b["d"][gg + 1] = row0[1] - row0[0], row1[1] - row1[0]
            b["ties"].append((gg, winner))
    else:
        b = _assemble(cases)
    return _finish(b)


def _labels(b, y, what):
    y = np.asarray(y).astype(np.int32)
    bad = np.nonzero(y != b["ey"])[0]
    assert bad.size == 0, f"{what}: {bad.size} labels differ from the oracle's, first at genes {bad[:5]} (workgroups {sorted(set((bad // 1900)[:5].tolist()))})"


def _every_path(nat, b):
    import torch

    model = nat.Model.from_tables(b["w"], vm.TRANS2)
    y, _ = model.viterbi(b["cptr"], b["gptr"], b["attr"], want_score=False)
    _labels(b, y, "Model.viterbi(want_score=False)")
    d_gp, d_at = torch.from_numpy(b["gptr"]).cuda(), torch.from_numpy(b["attr"]).cuda()
    n = b["n"]
    plan = nat.Plan(model, b["cptr"], 20, 1, True, device=0)
    d_y = torch.full((n,), 7, dtype=torch.int8, device="cuda:0")
    plan.viterbi_stats(reset=True)
    plan.run_viterbi(d_gp.data_ptr(), d_at.data_ptr(), d_y.data_ptr(), 0)
    st = plan.viterbi_stats()
    _labels(b, d_y.cpu().numpy(), "Plan.run_viterbi (vd_short)")
    plans = [nat.Plan(model, b["cptr"], 20, 1, True, device=0) for _ in range(2)]
    p = [torch.zeros(n, dtype=torch.float64, device="cuda:0") for _ in range(2)]
    yy = [torch.full((n,), 7, dtype=torch.int8, device="cuda:0") for _ in range(2)]
    plans[0].run_decode_pipelined(d_gp.data_ptr(), d_at.data_ptr(), p[0].data_ptr())
    plans[1].run_decode_pipelined(d_gp.data_ptr(), d_at.data_ptr(), p[1].data_ptr(), plans[0], yy[0].data_ptr())
    plans[1].flush_decode_pipelined(yy[1].data_ptr())
    torch.cuda.synchronize()
    for k in range(2):
        _labels(b, yy[k].cpu().numpy(), f"Plan.run_decode_pipelined[{k}]")
    return st


def test_runs_of_lanes_without_a_constant_map(nat):
    b = _batch("runs")
    assert sum(b["expect"]) >= 8 and b["expect"].count(False) >= 40
    _every_path(nat, b)


def test_waves_without_a_constant_lane_take_the_fallback(nat):
    b = _batch("waves")
    assert all(b["expect"])
    _every_path(nat, b)


def test_contig_boundaries_next_to_a_run(nat):
    b = _batch("cuts")
    assert not any(b["expect"])
    _every_path(nat, b)


def test_planted_ties_inside_and_behind_a_run(nat):
    b = _batch("ties")
    assert not any(b["expect"]) and len(b["ties"]) == 8
    for i, (g, _) in enumerate(b["ties"]):  # (the tie's lane: inside the run -- not constant; or the first constant lane behind it)
        lane = (g - i * N) // 8
        assert bool(b["blocks"][i]["constant"][lane]) == (i >= 4) and not b["blocks"][i]["constant"][lane - 1]
    st = _every_path(nat, b)
    # every planted decision lies inside the margin: its contig went through CRFsuite's own recursion
    assert st["contigs_redecoded"] >= len(b["ties"]), st
