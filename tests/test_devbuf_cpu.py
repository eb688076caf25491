"""The owning buffer type of the context (csrc/devbuf.h) without a GPU: DevBuf, PinBuf and the all-or-nothing group
reservation built as host code with the sanitizers over a counting allocator that can fail its k-th call
(tests/devbuf_host_check.cpp), and what csrc/api.hip may no longer spell once every buffer owns its memory."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hic_genome_assembler_amd", "csrc")


def _api():
    with open(os.path.join(CSRC, "api.hip")) as fh:
        return fh.read()


def test_devbuf_and_group_reservation_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "devbuf_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "devbuf_host_check.cpp"), "-o", exe])
    # an ordinary child process, nothing preloaded: a failed check, a block alive at the end, a double free or a sanitizer
    # report all end it with a status other than 0 or with text on stderr
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and done.stderr == "", done.stdout + done.stderr
    assert re.fullmatch(r"devbuf: OK \(\d+ allocations, \d+ frees\)\n", done.stdout), done.stdout


def test_devbuf_header_stands_alone():
    with open(os.path.join(CSRC, "devbuf.h")) as fh:
        includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", fh.read())
    assert "<hip/hip_runtime_api.h>" in includes
    assert all(inc.startswith("<") and (inc == "<hip/hip_runtime_api.h>" or "/" not in inc) for inc in includes), includes


def test_api_allocates_and_frees_only_through_the_buffer_type():
    api = _api()
    for spelt in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "free_dev"):
        assert spelt not in api, "csrc/api.hip spells %s: device and pinned memory belong to DevBuf / PinBuf" % spelt
    assert '#include "devbuf.h"' in api
    destroy = re.search(r"\nint hicmi_destroy\(hicmi_ctx\* c\)\n\{\n(.*?)\n\}\n", api, re.S).group(1)
    assert "delete c;" in destroy
    assert not re.findall(r"\bd_\w+", destroy), "hicmi_destroy names buffers again: tear-down is the members' business"


def test_context_keeps_no_separate_capacity_fields():
    ctx = re.search(r"\nstruct hicmi_ctx \{\n(.*?)\n\};\n", _api(), re.S).group(1)
    assert "DevBuf<" in ctx and "PinBuf<" in ctx
    fields = re.sub(r"//[^\n]*", "", ctx)
    assert not re.findall(r"\b\w+_cap\b", fields), re.findall(r"\b\w+_cap\b", fields)
    assert not re.findall(r"\*\s*d_\w+\s*=\s*nullptr", fields.replace("double* d_hx = nullptr", "")), \
        "a raw device pointer in the context (d_hx, a view of the selected HMM slot, is the one exception)"
