"""The tables of tests/reuse_cases.py held against the source, without a GPU: every device and pinned buffer of
struct hicmi_ctx is regrown by a family's cases (BUFFERS), every function of the driver that replaces the matrix or the
sums is reached by a replacer (REPLACER_SITES), and neither table names something that is gone.  A buffer or a site that
a later change adds fails here until a family or a replacer covers it."""
import os
import re

import numpy as np

import reuse_cases as rc

CSRC = os.path.join(rc.ROOT, "hic_genome_assembler_amd", "csrc")
SOURCES = ("api.hip", "api_pairs.inc", "api_links.inc")
BUFFER = re.compile(r"\b(?:DevBuf|PinBuf)<[^;>]+>\s+([^;()]+);")
NESTED = re.compile(r"\bstruct\s+(\w+)\s*\{([^{}]*)\}\s*;")
FUNCTION = re.compile(r"^(?:static\s+)?(?:inline\s+)?(?:int|void|bool|int64_t|double|hipError_t)\s+(\w+)\s*\(", re.M)
SITE = re.compile(r"\b(?:drop_matrix_state|own_matrix|ice_matrix_changed|forget_matrix_derived)\s*\(\s*c\b|c->dC\s*=(?!=)"
                  r"|\bupload\s*\(\s*c\s*,\s*c->d_np\b")


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def struct_buffers(text):
    """The DevBuf<> and PinBuf<> members of struct hicmi_ctx in ``text``; those of a struct nested in it under the name
    of the member of that type ("hslot.d_x")."""
    body = re.search(r"^struct hicmi_ctx \{\n(.*?)^\};", text, re.M | re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = []
    for kind, inner in NESTED.findall(body):
        holder = re.search(r"\b%s\s+(\w+)" % kind, NESTED.sub("", body)).group(1)
        names += [holder + "." + n for n in _declared(inner)]
    return names + _declared(NESTED.sub("", body))


def _declared(body):
    return [n.strip() for decl in BUFFER.findall(body) for n in decl.split(",")]


def replacer_sites(texts):
    """The functions of ``texts`` that drop or install a matrix, say that it changed, assign dC or upload into d_np."""
    found = set()
    for text in texts:
        starts = [(m.start(), m.group(1)) for m in FUNCTION.finditer(text)]
        for m in SITE.finditer(re.sub(r"//[^\n]*", lambda c: " " * len(c.group(0)), text)):
            inside = [name for pos, name in starts if pos <= m.start()]
            assert inside, "a matrix site before the first function"
            found.add(inside[-1])
    return found


def test_every_buffer_of_the_context_is_regrown_by_a_family():
    members = struct_buffers(_read("api.hip"))
    assert len(members) == len(set(members)) > 100
    assert sorted(set(members) - set(rc.BUFFERS)) == [], "buffers of hicmi_ctx that no family of reuse_cases.BUFFERS regrows"
    assert sorted(set(rc.BUFFERS) - set(members)) == [], "reuse_cases.BUFFERS names buffers that hicmi_ctx does not have"
    for member, families in rc.BUFFERS.items():
        assert families and set(families) <= set(rc.FAMILIES), member
    assert {f for families in rc.BUFFERS.values() for f in families} == set(rc.FAMILIES)     # no family without a buffer


def test_a_new_buffer_or_a_dropped_line_is_noticed():
    text = _read("api.hip")
    probe = text.replace("    DevBuf<double> d_zraw;\n", "    DevBuf<double> d_zraw;\n    DevBuf<int> d_probe;\n")
    assert probe != text and set(struct_buffers(probe)) - set(rc.BUFFERS) == {"d_probe"}
    two = text.replace("    DevBuf<double> d_zraw;\n", "    DevBuf<double> d_zraw; PinBuf<char> pin_a, pin_b;\n")
    assert set(struct_buffers(two)) - set(rc.BUFFERS) == {"pin_a", "pin_b"}
    nested = text.replace("struct HmmSlot { DevBuf<double> d_x;", "struct HmmSlot { DevBuf<double> d_x; DevBuf<int> d_y;")
    assert nested != text and set(struct_buffers(nested)) - set(rc.BUFFERS) == {"hslot.d_y"}
    assert "d_zraw" in struct_buffers(text) and "hslot.d_x" in struct_buffers(text) and "d_x" in struct_buffers(text)


def test_every_matrix_site_is_reached_by_a_replacer():
    sites = replacer_sites([_read(name) for name in SOURCES])
    assert sorted(sites - set(rc.REPLACER_SITES)) == [], "functions that replace the matrix or the sums without a replacer"
    assert sorted(set(rc.REPLACER_SITES) - sites) == [], "reuse_cases.REPLACER_SITES names functions that replace nothing"
    names = [name for name, _apply in rc.REPLACERS]
    assert len(names) == len(set(names))
    for site, replacers in rc.REPLACER_SITES.items():
        assert replacers and set(replacers) <= set(names), site
    assert {r for replacers in rc.REPLACER_SITES.values() for r in replacers} == set(names)    # no replacer without a site


def test_a_new_matrix_site_is_noticed():
    text = "int hicmi_probe(hicmi_ctx* c)\n{\n    // drop_matrix_state(c) in a comment is none\n    c->dC = nullptr;\n    return 0;\n}\n"
    assert replacer_sites([text]) == {"hicmi_probe"}
    assert replacer_sites(["int f(hicmi_ctx* c)\n{\n    if (c->dC == nullptr) return 1;\n    return own_matrix_rows(c);\n}\n"]) == set()
    assert replacer_sites(["void g(hicmi_ctx* c)\n{\n    upload(c, c->d_np, p, 8);\n}\nint h(hicmi_ctx* c)\n{\n    return 0;\n}\n"]) == {"g"}


def test_the_dependents_and_their_chain():
    from hic_genome_assembler_amd import _lib
    names = [name for name, _step, _call in rc.DEPENDENTS]
    assert len(names) == len(set(names)) == 24
    for name, step, _call in rc.DEPENDENTS:
        assert callable(getattr(_lib.Context, name)) and callable(getattr(_lib.Context, step)), name
        assert step in rc.CHAIN and rc.REFUSALS[step][-1] == step
    # the words of the refusals are the library's
    source = _read("api.hip")
    for step, words in rc.NOT_RUN.items():
        assert '"%s"' % words in source, step
    # the chain's inputs fit every map the replacers leave (96 bins or more) and are an arrangement with two scaffolds left
    assert rc.SEL.max() < 96 and int(rc.LENS.sum()) == len(rc.SEL) and (rc.STARTS + rc.LENS).max() == len(rc.SEL)
    assert sorted(rc.IDS.tolist() + rc.NEW_IDS.tolist()) == list(range(len(rc.LENS))) and len(rc.REV) == len(rc.IDS)
    assert max(rc.CUTS) < 96 and all(sorted(p.tolist()) == list(range(len(rc.SEL))) for p in rc.PERMS)


def test_the_cases_shrink_and_regrow():
    first, small, large = rc.pair_cases()
    assert all(s < f < g for s, f, g in zip(small.measures(), first.measures(), large.measures()))
    assert all(len(c.pairs[0]) < 20000 for c in (first, small, large))
    sizes, tables, pairs = rc.stale_pairs()
    assert int(np.ceil(sizes / 500).sum()) >= 96 and int(np.ceil(tables[3] / 500).sum()) >= 96
    assert rc.SIZES == (192, 320, 192) and max(rc.SIZES) <= 320


def test_marked_outputs_sees_a_write():
    from hic_genome_assembler_amd import _lib
    with rc.marked_outputs() as marks:
        a = _lib.np.empty((3, 2), np.float64)
        b = _lib.np.empty(0, np.int32)
        assert _lib.np.zeros(2).tolist() == [0.0, 0.0] and marks.untouched()
        a[1, 1] = 0.0
        assert not marks.untouched() and b.size == 0
    with rc.marked_outputs() as marks:                         # arrays made with zeros and scalars count from the call on
        z, x, k = _lib.np.zeros(3, np.int64), _lib.c_dbl(float("nan")), _lib.c_i64()
        z[0] = 7
        assert _lib._ptr(z) is not None and _lib._ptr(None) is None and marks.untouched()
        x.value = float("nan")
        assert marks.untouched() and k.value == 0 and isinstance(x.value, float)
        z[1] = 1
        assert not marks.untouched()
    with rc.marked_outputs() as marks:
        k = _lib.c_i64(4)
        k.value += 1
        assert not marks.untouched()
    import ctypes
    assert _lib.np is np and _lib.c_i64 is ctypes.c_int64 and _lib.c_dbl is ctypes.c_double and _lib._ptr(None) is None


def test_the_fake_context_forgets_with_the_matrix():
    """tests/fake_context.py models the guards: what the library refuses after a new matrix, it refuses."""
    import pytest
    from fake_context import OracleContext, OracleError
    ctx = OracleContext()
    c = np.arange(36, dtype=np.float64).reshape(6, 6) + 1.0
    c = c + c.T
    sel, starts, lens = np.arange(6), [0, 3], [3, 3]

    def build():
        ctx.rank_matrix(np.arange(6))
        ctx.p2_select(sel)
        ctx.p2_layout(starts, lens)
        ctx.p2_set_arrangement([0, 1], [0, 1])

    ctx.set_contacts(c)
    build()
    ctx.rank_rows(), ctx.p2_total(), ctx.p2_arrangement_total()
    for replace in (lambda: ctx.set_contacts(c * 2.0), lambda: ctx.compact([0, 1, 2, 3, 5])):
        replace()
        for call, words in ((ctx.rank_rows, "hicmi_rank_matrix has not run"), (ctx.p2_total, "hicmi_p2_select has not run"),
                            (lambda: ctx.p2_layout([0], [2]), "hicmi_p2_select has not run"),
                            (lambda: ctx.p2_set_arrangement([0], [0]), "hicmi_p2_layout has not run"),
                            (ctx.p2_arrangement_total, "hicmi_p2_set_arrangement has not run")):
            with pytest.raises(OracleError, match=words):
                call()
        sel = np.arange(5)
        ctx.set_contacts(c)
        build()
    ctx.set_row_sums(np.ones(6), np.arange(6) + 1.0)
    with pytest.raises(OracleError, match="hicmi_rank_matrix has not run"):
        ctx.rank_rows()
    assert ctx.p2_arrangement_total() > 0                      # other sums under the same matrix: Part 2 stands
