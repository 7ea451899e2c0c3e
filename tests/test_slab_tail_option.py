"""Option "slab_tail" of mdbn_set_option against the library source and the public header (no GPU needed): what
tests/test_knob_registry.py checks for the knobs of tests/_knobs.py, for the option that mdbn_set_option hands to
set_plane_kernel_option.  The GPU tests that drive it are tests/test_gpu_slab_tail.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = os.path.join(ROOT, "mdbn_amd", "csrc", "mdbn_capi.hip")
CAPI_INTERNAL = os.path.join(ROOT, "mdbn_amd", "csrc", "mdbn_capi_internal.h")
HEADER = os.path.join(ROOT, "include", "mdbn_hip.h")


def _helper_body():
    src = open(CAPI).read()
    at = src.index("static bool set_plane_kernel_option(")
    return src[at:src.index("\n}\n", at)]


def test_the_option_is_a_flag_of_the_context_and_set_option_reaches_it():
    body = _helper_body()
    names = re.findall(r'strcmp\(name, "([^"]+)"\) == 0', body)
    assert names == ["slab_tail"], names                       # a name added there needs its checks added here
    assert re.search(r"ctx->opt\.slab_tail = value != 0;", body)          # every integer is taken as a flag: nothing to refuse
    src = open(CAPI).read()
    at = src.index("int mdbn_set_option(mdbn_ctx* ctx")
    assert "if (set_plane_kernel_option(ctx, name, value)) return MDBN_OK;" in src[at:src.index("\n}\n", at)]


def test_a_fresh_context_has_it_on():
    src = open(CAPI_INTERNAL).read()
    body = src[src.index("struct Options {"):]
    assert re.search(r"^\s+int slab_tail = 1;", body[:body.index("};")], re.M)


def test_it_is_documented_in_the_public_header():
    src = open(HEADER).read()
    assert '"slab_tail" (default 1)' in src[src.index("Tuning knobs, PER CONTEXT"):src.index("int  mdbn_set_option(")]
