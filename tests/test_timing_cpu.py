"""Without a GPU: the counting restatement of SciPy's nn_chain (tests/nnchain_count_reference.py) that the GPU tests of
the nn-chain counters compare with is pinned against SciPy, against the oracle's C port and against recorded counts; and
the family table of csrc/api.hip fits what _lib.Context._timing_one and bench.py expect of it."""
import os
import re

import numpy as np
import pytest

import nnchain_count_reference as ref

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

# (bins, seed of the map): the maps of the nn-chain parity tests
SEEDS = {5: 0, 65: 4, 300: 5, 1025: 6}
# recorded once from nn_chain_counted on orc.to_distance(map): (merges, chain steps, columns visited)
RECORDED = {("random", 5): (4, 10, 35), ("random", 65): (64, 175, 6115), ("random", 300): (299, 861, 131444),
            ("random", 1025): (1024, 2952, 1544585),
            ("ties", 5): (4, 8, 28), ("ties", 65): (64, 180, 6253), ("ties", 300): (299, 863, 134244),
            ("ties", 1025): (1024, 3018, 1566920)}


@pytest.fixture(scope="module")
def orc():
    import hic_oracle
    return hic_oracle


def _distance(orc, kind, n):
    c = ref.random_contacts(n, SEEDS[n]) if kind == "random" else ref.all_ties_contacts(n, SEEDS[n])
    return orc.to_distance(c)


@pytest.mark.parametrize("n", sorted(SEEDS))
@pytest.mark.parametrize("kind", ["random", "ties"])
def test_counting_reference_is_scipys_nn_chain(orc, kind, n):
    """Raw merges: the oracle's C port of nn_chain, bit for bit (slots, heights, sizes, merge ORDER - so the chain that
    was walked is the same).  Heights: SciPy's own linkage.  Counts: the recorded ones."""
    from scipy.cluster.hierarchy import linkage
    d = _distance(orc, kind, n)
    zraw, steps, columns = ref.nn_chain_counted(d)
    assert np.array_equal(zraw, orc.nn_chain_raw(d))
    z = linkage(d[np.triu_indices(n, 1)], "average")
    assert np.array_equal(np.sort(zraw[:, 2], kind="stable"), z[:, 2])
    assert np.array_equal(orc.label_linkage(zraw, n), z)
    assert (len(zraw), steps, columns) == RECORDED[(kind, n)]


def test_counting_reference_bounds():
    """A 2-bin map is one merge in two steps (start, confirm) over two live clusters; every merge ends with a step of
    its own and the first needs one more; a step visits at most n columns."""
    zraw, steps, columns = ref.nn_chain_counted(np.array([[0.0, 3.0], [7.0, 0.0]]))
    assert zraw.tolist() == [[0.0, 1.0, 3.0, 2.0]] and (steps, columns) == (2, 4)
    assert ref.nn_chain_counted(np.zeros((1, 1)))[1:] == (0, 0)
    for (_kind, n), (merges, steps, columns) in RECORDED.items():
        assert merges == n - 1 and merges < steps and columns <= steps * n


def test_counting_reference_reads_the_upper_triangle_only(orc):
    d = _distance(orc, "random", 65)
    assert not np.array_equal(d, d.T)                    # the project's distance is not symmetric (row sums differ)
    low = np.tril(np.full_like(d, 123.0), -1)
    a, b = ref.nn_chain_counted(d), ref.nn_chain_counted(np.triu(d, 1) + low)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def test_the_all_ties_map_is_the_parity_tests():
    """all_ties_contacts must be what test_upgma_without_neighbour_cache_bit_exact builds: drawn from the generator
    after the random map."""
    n, seed = 65, 4
    rng = np.random.default_rng(seed)
    c = rng.random((n, n)) + 0.01
    c = c + c.T
    ties = rng.integers(1, 4, size=(n, n)).astype(np.float64)
    ties = np.triu(ties, 1) + np.triu(ties, 1).T + np.eye(n)
    assert np.array_equal(ref.random_contacts(n, seed), c)
    assert np.array_equal(ref.all_ties_contacts(n, seed), ties)
    assert len(np.unique(ties)) == 3


# ------------------------------------------------------------------------------------------------ the family table
def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def _family_table():
    src = _read("hic_genome_assembler_amd", "csrc", "api.hip")
    enum = re.search(r"enum Family \{(.*?)\};", src, re.S).group(1)
    ids = [t.strip() for t in enum.split(",") if t.strip()]
    table = re.search(r"kFamilyNames\[F_COUNT\] = \{(.*?)\};", src, re.S).group(1)
    names = re.findall(r'"([^"]*)"', re.sub(r"//[^\n]*", "", table))
    return src, ids, names


def test_family_table_fits_the_python_side():
    """_lib.Context._timing_one hands hicmi_timing_get room for 32 families and 1,024 bytes of ';'-joined names."""
    _src, ids, names = _family_table()
    assert ids[-1] == "F_COUNT" and len(ids) - 1 == len(names)
    lib = _read("hic_genome_assembler_amd", "_lib.py")
    body = lib[lib.index("def _timing_one"):]
    assert "create_string_buffer(1024)" in body and "np.zeros(32, np.float64)" in body and ", 32,\n" in body
    assert len(names) <= 32
    assert len(";".join(names)) + 1 <= 1024
    assert len(set(names)) == len(names)
    assert all(nm and ";" not in nm for nm in names)


def test_family_names_bench_looks_up_exist():
    _src, _ids, names = _family_table()
    bench = _read("bench.py")
    assert 'fam == "nnchain"' in bench and "nnchain" in names
    assert 'k.startswith("p2_")' in bench and any(nm.startswith("p2_") for nm in names)
    for looked_up in re.findall(r'timing(?:\.get\(|\[)"(\w+)"', bench):
        assert looked_up in names, looked_up
    assert "p2_window_G_flops" in names and "p2_window_G" in names
    pmc = bench[bench.index("PMC_KERNELS = {"):bench.index("def make_bins")]
    for fam in re.findall(r'"(\w+)": \(', pmc):
        assert fam in names, fam


def test_few_launch_set_of_mode_2_is_what_the_header_says():
    """Timed::on(): mode 2 times the families up to rank_invert and those from presort_rows on, except the flops
    counter, which never launches.  include/hicmi.h names them."""
    src, ids, names = _family_table()
    on = re.search(r"bool on\(\) const \{ return (.*?); \}", src).group(1)
    assert on == "c->timing == 1 || (c->timing == 2 && (fam <= F_RANK_INVERT || fam >= F_PRESORT))"
    few = [names[k] for k, f in enumerate(ids[:-1]) if k <= ids.index("F_RANK_INVERT") or k >= ids.index("F_PRESORT")]
    assert few == ["row_sums", "build_w", "nnchain", "sort_rows", "rank_invert", "presort_rows", "rank_relabel",
                   "rank_rows_tied", "p2_window_G_flops"]
    header = _read("include", "hicmi.h")
    comment = header[header.index("hicmi_timing_enable: 0 = off"):header.index("int hicmi_timing_reset")]
    for nm in few[:-1]:
        assert nm in comment, nm


# ------------------------------------------------------------------------------ a plain benchmark run and --full
ALL_LEGS = {"table", "32k", "64k", "cpu_baseline", "e2e"}


@pytest.fixture(scope="module")
def bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hicmi_bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                        # stdlib imports only: torch and the library are loaded in main()
    return mod


def _legs(bench, argv, world=1):
    legs = bench.extra_legs(bench.arg_parser().parse_args(argv), world)
    assert set(legs) == ALL_LEGS
    return {k for k, on in legs.items() if on}


@pytest.mark.parametrize("argv", [[], ["--gpus", "1", "--steps", "3", "--warmup", "1"], ["--dump-outputs", "somewhere"],
                                  ["--part1-only"], ["--bins", "32000"], ["--kernel-times", "all"]])
def test_a_plain_bench_run_makes_no_measurement_of_its_own(bench, argv):
    """Without --full nothing beside the warm-up and the timed steps runs, whatever else is asked for."""
    assert _legs(bench, argv) == set()
    assert _legs(bench, argv, world=4) == set()


def test_full_bench_run_makes_what_a_default_run_made(bench):
    """--full: every measurement; a --no-* option leaves its own out (and --no-cpu-baseline the CLI runs with it, as
    before); a map size is not measured twice; Part 2's sizes are not run beside --part1-only; one process only."""
    assert _legs(bench, ["--full"]) == ALL_LEGS
    assert _legs(bench, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"]) == ALL_LEGS
    assert _legs(bench, ["--full", "--no-table"]) == ALL_LEGS - {"table"}
    assert _legs(bench, ["--full", "--no-32k"]) == ALL_LEGS - {"32k"}
    assert _legs(bench, ["--full", "--no-64k"]) == ALL_LEGS - {"64k"}
    assert _legs(bench, ["--full", "--no-e2e"]) == ALL_LEGS - {"e2e"}
    assert _legs(bench, ["--full", "--no-cpu-baseline"]) == ALL_LEGS - {"cpu_baseline", "e2e"}
    assert _legs(bench, ["--full", "--bins", "32000"]) == ALL_LEGS - {"32k"}
    assert _legs(bench, ["--full", "--bins", "64000"]) == ALL_LEGS - {"64k"}
    assert _legs(bench, ["--full", "--part1-only"]) == ALL_LEGS - {"32k", "64k"}
    assert _legs(bench, ["--full"], world=2) == set()
    assert _legs(bench, ["--full", "--no-cpu-baseline", "--no-32k", "--no-64k", "--no-e2e", "--no-table"]) == set()


def test_every_extra_measurement_of_bench_is_behind_its_leg():
    """main() starts each of them in one place, directly under the test of its leg."""
    src = _read("bench.py")
    main = src[src.index("def main():"):]
    for leg, call in (("table", "timed_run(job, 1, 0, 1,"), ("32k", "side_job(32000,"), ("64k", "side_job(64000,"),
                      ("cpu_baseline", "cpu_baseline(args.cpu_sample_bins,"), ("e2e", "e2e_cli(2000,"),
                      ("e2e", "e2e_cli_cached(16000,")):
        assert main.count(call) == 1, call
        guard = main.rindex("if legs[", 0, main.index(call))
        assert main[guard:].startswith('if legs["%s"]:' % leg), call
        between = main[guard:main.index(call)]
        assert "\n    if " not in between and "\nif " not in between, call      # no other top-level branch in between
    # timed_run: the headline's, the table's, side_job's own; side_job: its definition and the two sizes
    assert main.count("timed_run(") == 3 and main.count("side_job(") == 3
