"""The cases of tests/insertion_reference.py reach the branches they are named after - shown from the oracle alone.

tests/test_gpu_insertion.py compares the device's insertion phase and scan loops with Part2Oracle on these cases.  A
case is only worth its GPU time if the oracle's own literal costs put it on the intended branch of k_part2_insert.hip:
how many candidates lie within the short lists' 1e-9 band of the best (one: the direct take; more than INS_MAXC = 8: a host
step in the middle of the queue; 9 - 16 for a one-bin scaffold: the twin rule), whether every cost is NaN, whether
all are bit-equal.  A smooth random map has one or two near-top candidates at every step and meets none of the
conditions below except the generic ones.
"""
import numpy as np
import pytest

import insertion_reference as ir

INS_MAXC = 8


def _near(name):
    return [ir.near_top_count(s.costs) for s in ir.reference(name).steps]


def test_generic_has_direct_steps_and_one_bin_twins():
    case, ref = ir.case_generic(), ir.reference("generic")
    near = _near("generic")
    assert 1 in near
    assert any(m == 2 and case.lens[s.new_id] == 1 for m, s in zip(near, ref.steps))
    assert all(m <= 2 for m in near)
    assert all(s.decided for s in ref.steps)


@pytest.mark.parametrize("bins", [2, 1])
def test_isolated_scaffold_ties_four_ways(bins):
    name = "isolated-%d-bin" % bins
    case, ref = ir.ALL_CASES[name](), ir.reference(name)
    hits = [s for s in ref.steps if ir.near_top_count(s.costs) == 4]
    assert len(hits) == 1
    s = hits[0]
    assert case.lens[s.new_id] == bins
    S = len(s.ids_before)
    top = s.costs.max()
    tied = np.flatnonzero(s.costs >= top - abs(top) * ir.NEAR_TOP)
    assert tied.tolist() == [0, 1, 2 * S, 2 * S + 1]          # both ends, both orientations


def test_block_diagonal_overflows_the_short_list_at_every_step():
    ref = ir.reference("block-diagonal")
    near = _near("block-diagonal")
    assert near == [2 * (len(s.ids_before) + 1) for s in ref.steps]          # every candidate ties
    assert all(m > INS_MAXC for m in near)
    # two or more literal values among the tied: the first strict maximum is decided by the arithmetic, not by position
    distinct = [len(set(s.costs.tolist())) for s in ref.steps]
    assert max(distinct) >= 2
    assert any(s.gap != 0 or s.rev != 0 for s in ref.steps)


def test_block_diagonal_small_keeps_lists_of_9_to_16_for_one_bin_scaffolds():
    case, ref = ir.case_block_diagonal_small(), ir.reference("block-diagonal-small")
    near = _near("block-diagonal-small")
    assert [len(s.ids_before) for s in ref.steps] == [4, 5, 6, 7, 8]
    assert all(case.lens[s.new_id] == 1 for s in ref.steps)
    assert all(INS_MAXC < m <= 2 * INS_MAXC for m in near[:4])
    assert near[4] == 18                                      # beyond twice the cap: the device declines this step


def test_no_contacts_scores_nan_everywhere():
    ref = ir.reference("no-contacts")
    for s in ref.steps:
        assert np.isnan(s.costs).all()
        assert ir.near_top_count(s.costs) == 0
        assert (s.gap, s.rev, s.best, s.decided) == (0, 0, 0.0, False)


def test_constant_matrix_makes_every_candidate_bit_equal():
    ref = ir.reference("constant")
    for s in ref.steps:
        assert len(set(s.costs.tolist())) == 1 and s.costs[0] > 0.0
        assert (s.gap, s.rev, s.decided) == (0, 0, True)


def test_quantised_map_has_exact_zeros_and_integer_ties():
    case, ref = ir.case_quantised(), ir.reference("quantised")
    sc = ir.scaffold_of_bin(case.lens)
    between = case.mat[sc[:, None] != sc[None, :]]
    assert np.count_nonzero(between == 0.0) > between.size // 2
    assert np.array_equal(2.0 * case.mat, np.round(2.0 * case.mat))
    assert max(_near("quantised")) >= 2
    assert any(len(set(s.costs.tolist())) < len(s.costs) for s in ref.steps)


def test_256_scaffolds_cross_one_block_of_lanes():
    case, ref = ir.case_256_scaffolds(), ir.reference("256-scaffolds")
    sizes = [len(s.ids_before) for s in ref.steps]
    assert sizes == list(range(250, 262))
    assert 255 in sizes and 256 in sizes and 257 in sizes    # g = tid; g < S and i = tid; i < 2 (S + 1) take a second trip
    assert set(case.lens) == {1, 2}
    assert any(c.rev for c in ref.steps) and any(r for r in case.rev0)
    assert len({s.gap for s in ref.steps}) > 1


def test_8192_bin_case_straddles_both_staging_limits():
    lens = ir.BINS_8192_LENS
    ids0, new_ids = (0, 1, 2), (3, 4, 5)
    n_arr = [sum(lens[i] for i in ids0) + sum(lens[i] for i in new_ids[:t]) for t in range(3)]
    assert n_arr == [8191, 8192, 8193]                        # STRADDLE staged, staged, read from L2
    assert [n + lens[i] for n, i in zip(n_arr, new_ids)] == [8192, 8193, 8195]      # literal pass staged, then streamed


@pytest.mark.parametrize("name", sorted(ir.SCAN_CASES))
def test_scan_cases_run_more_than_one_round(name):
    ref = ir.scan_reference(name)
    if name.startswith("constant"):
        assert ref.rounds == 1
        assert np.array_equal(ref.ids, ref.ids0) and np.array_equal(ref.rev, ref.rev0) and ref.best == ref.best0
    else:
        assert ref.rounds >= 2
        assert ref.best > ref.best0
        assert not (np.array_equal(ref.ids, ref.ids0) and np.array_equal(ref.rev, ref.rev0))


def test_enumeration_mapping_is_a_permutation_that_follows_the_flips():
    s = ir.reference("generic").steps[0]
    tagged = s._replace(costs=np.arange(len(s.costs), dtype=np.float64))
    assert ir.by_gap_rev(tagged).tolist() == [0, 1, 3, 2, 4, 5, 7, 6, 8, 9]
    assert ir.by_gap_rev(tagged, enter_flipped=True).tolist() == [1, 0, 2, 3, 5, 4, 6, 7, 9, 8]


def test_entering_flipped_changes_the_winner_among_bit_equal_twins():
    case = ir.case_block_diagonal_small()
    plus, minus = ir.run_insertion(case), ir.run_insertion(case, enter_flipped=True)
    assert [s.rev for s in plus.steps] == [0] * 5 and [s.rev for s in minus.steps] == [1] * 5
