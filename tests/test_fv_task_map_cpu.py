"""Task order of fv_mlp_k<KT, true> (csrc/feature_volume.hip: fv_skip_task), read through the host-only entry points the kernel shares
its code with: idh_feature_volume_grid (the launcher's grid) and idh_feature_volume_skip_task (ntasks, grid, block, wave, round) -> task or -1.
Wave w of a workgroup takes sub-slot (w + round) & 7 of the workgroup's eight tasks of a round; every task must be visited exactly once, also
where the last round is ragged (a rotated sub-slot past ntasks is skipped, lower ones of the same workgroup are not)."""
import pytest

from implicit_depth_amd import _lib

NTASKS = [1, 7, 8, 100, 2047, 2048, 2049, 4096 + 5, 24576]


def _visits(L, ntasks, grid):
    """{(block, wave): [task or -1 per round]} over every round that can hold a task, plus one round past the end."""
    rounds = -(-ntasks // (grid * 8))
    return {(b, w): [L.idh_feature_volume_skip_task(ntasks, grid, b, w, r) for r in range(rounds + 1)] for b in range(grid) for w in range(8)}, rounds


@pytest.mark.parametrize("ntasks", NTASKS)
def test_every_task_exactly_once(ntasks):
    L = _lib.lib()
    grid = L.idh_feature_volume_grid(ntasks)
    assert grid == min(256, (ntasks + 7) // 8)
    if ntasks == 100:
        assert grid == 13  # (not a multiple of 8: the XCD remap gives five XCDs two workgroups and three XCDs one)
    visits, rounds = _visits(L, ntasks, grid)
    seen = sorted(t for v in visits.values() for t in v if t >= 0)
    assert seen == list(range(ntasks))
    for (b, w), v in visits.items():
        assert v[rounds] == -1, (b, w)  # nothing past the last round
        assert all(-1 <= t < ntasks for t in v)
    # the workgroup's task set per round is the static mapping's: eight consecutive tasks from a multiple of 8 (XCD / L2 locality unchanged)
    for b in range(grid):
        for r in range(rounds):
            got = sorted(visits[(b, w)][r] for w in range(8) if visits[(b, w)][r] >= 0)
            if got:
                base = got[0] // 8 * 8
                assert got == list(range(base, min(base + 8, ntasks))), (b, r, got)
                assert r * grid * 8 <= base < (r + 1) * grid * 8


def test_ragged_last_round_skips_a_slot_and_goes_on():
    """ntasks = 4096 + 5 on 256 workgroups: in round 2 only sub-slots 0..4 of one workgroup exist; the waves that hold them there are
    (sub - 2) & 7 = 6, 7, 0, 1, 2, so waves 0..2 take a task while waves 3..5, which come before waves 6 and 7, take none."""
    L = _lib.lib()
    ntasks, grid = 4096 + 5, 256
    last = {w: [L.idh_feature_volume_skip_task(ntasks, grid, b, w, 2) for b in range(grid)] for w in range(8)}
    holders = {w: [t for t in v if t >= 0] for w, v in last.items()}
    assert {w: len(h) for w, h in holders.items()} == {0: 1, 1: 1, 2: 1, 3: 0, 4: 0, 5: 0, 6: 1, 7: 1}
    assert sorted(t for h in holders.values() for t in h) == list(range(4096, 4101))
    assert holders[6] == [4096] and holders[2] == [4100]


def test_each_wave_meets_all_residues_at_the_benchmark_shape():
    """32 frames x 768 tiles, G = 1: 12 rounds of 2048 tasks.  With the static stride task % 8 == wave in every round; rotated, every wave meets all
    eight residues (= all eight x-blocks of a 128-pixel image row), the first eight rounds once each."""
    L = _lib.lib()
    ntasks, grid = 24576, 256
    assert L.idh_feature_volume_grid(ntasks) == grid
    for b in range(grid):
        for w in range(8):
            tasks = [L.idh_feature_volume_skip_task(ntasks, grid, b, w, r) for r in range(12)]
            assert min(tasks) >= 0
            assert {t % 8 for t in tasks} == set(range(8)), (b, w)
            assert sorted(t % 8 for t in tasks[:8]) == list(range(8)), (b, w)


def test_arguments_out_of_range():
    L = _lib.lib()
    assert L.idh_feature_volume_grid(0) == 0 and L.idh_feature_volume_grid(-3) == 0
    assert L.idh_feature_volume_grid(1 << 40) == 256
    for bad in [(0, 1, 0, 0, 0), (8, 0, 0, 0, 0), (8, 1, -1, 0, 0), (8, 1, 1, 0, 0), (8, 1, 0, -1, 0), (8, 1, 0, 8, 0), (8, 1, 0, 0, -1)]:
        assert L.idh_feature_volume_skip_task(*bad) == -1, bad
    assert L.idh_feature_volume_skip_task(8, 1, 0, 3, 0) == 3
    # past 2^31 tasks the index stays exact (64-bit)
    n = (1 << 33) + 3
    r = n // (256 * 8)
    assert L.idh_feature_volume_skip_task(n, 256, 0, (0 - r) & 7, r) == r * 2048
