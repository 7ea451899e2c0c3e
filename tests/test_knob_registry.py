"""The tuning knobs of mdbn_set_option against their registry (tests/_knobs.py) and the public header, and the build's source
list against the #include graph of the HIP sources (no GPU needed)."""
import ast
import os
import re
import shutil

import pytest

from _knobs import KNOBS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CAPI = os.path.join(ROOT, "mdbn_amd", "csrc", "mdbn_capi.hip")
CAPI_INTERNAL = os.path.join(ROOT, "mdbn_amd", "csrc", "mdbn_capi_internal.h")
HEADER = os.path.join(ROOT, "include", "mdbn_hip.h")


def _set_option_body():
    src = open(CAPI).read()
    at = src.index("int mdbn_set_option(mdbn_ctx* ctx")
    return src[at:src.index("\n}\n", at)]


def _library_knobs():
    """{option name: Options field it writes} parsed from mdbn_set_option."""
    out = {}
    for block in re.split(r"\n    if \(strcmp\(name, ", _set_option_body())[1:]:
        name = re.match(r'"([^"]+)"\) == 0\)', block).group(1)
        field = re.search(r"ctx->opt\.(\w+) =", block)
        out[name] = field.group(1) if field else None
    return out


def _options_defaults():
    """{Options field: default} parsed from struct Options of mdbn_capi_internal.h."""
    src = open(CAPI_INTERNAL).read()
    body = src[src.index("struct Options {"):]
    body = body[:body.index("};")]
    out = {}
    for m in re.finditer(r"^\s+(?:int|int64_t) (\w+) = ([^;]+);", body, re.M):
        expr = m.group(2).replace("(int64_t)", "").replace("ll", "")
        out[m.group(1)] = eval(expr, {})          # integer literals and shifts only
    return out


def test_every_library_knob_is_in_the_registry_and_nothing_else():
    lib = _library_knobs()
    assert len(lib) == len(re.findall(r'strcmp\(name, "', _set_option_body())), "a knob name appears twice"
    missing, stale = sorted(set(lib) - set(KNOBS)), sorted(set(KNOBS) - set(lib))
    assert not missing, "knobs of mdbn_set_option without a tests/_knobs.py entry (and so without a test): %s" % missing
    assert not stale, "tests/_knobs.py entries mdbn_set_option does not know: %s" % stale


def test_registry_defaults_are_the_fresh_context_options():
    lib, defaults = _library_knobs(), _options_defaults()
    for name, field in lib.items():
        assert field in defaults, (name, field)
        assert KNOBS[name]["default"] == defaults[field], name
        assert KNOBS[name]["default"] in KNOBS[name]["valid"], name


def test_registry_entries_are_well_formed():
    for name, e in KNOBS.items():
        assert set(e) == {"default", "valid", "invalid", "tests"}, name
        assert e["valid"] and e["tests"], name
        assert not set(e["valid"]) & set(e["invalid"]), name
        assert all(-(1 << 63) <= v < (1 << 63) for v in e["valid"] + e["invalid"]), name      # (int64_t on the C side)


def _test_functions(path):
    tree = ast.parse(open(path).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}


def test_every_referenced_test_exists():
    cache = {}
    for name, e in KNOBS.items():
        for node in e["tests"]:
            fname, _, func = node.partition("::")
            path = os.path.join(TESTS, fname)
            assert os.path.exists(path), "%s: %s does not exist" % (name, fname)
            if path not in cache:
                cache[path] = _test_functions(path)
            assert func.startswith("test_") and func in cache[path], "%s: no test %s in %s" % (name, func, fname)


def test_every_knob_is_documented_in_the_public_header():
    src = open(HEADER).read()
    block = src[src.index("Tuning knobs, PER CONTEXT"):src.index("int  mdbn_set_option(")]
    undocumented = sorted(n for n in _library_knobs() if '"%s"' % n not in block)
    assert not undocumented, "knobs missing from the knob comment of include/mdbn_hip.h: %s" % undocumented


# ------------------------------------------------------------------ build inputs


def _includes_reachable(csrc, sources):
    """Every file (relative to csrc) reachable through #include "..." from the given sources."""
    seen, todo = set(), list(sources)
    while todo:
        f = os.path.normpath(todo.pop())
        if f in seen:
            continue
        seen.add(f)
        here = os.path.dirname(f)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(csrc, f)).read(), re.M):
            todo.append(os.path.join(here, inc))
    return seen


def test_every_included_file_is_a_build_input():
    from mdbn_amd import build
    listed = {os.path.normpath(f) for f in build.SOURCES + build.HEADERS}
    reach = _includes_reachable(build.CSRC, build.SOURCES)
    missing = sorted(reach - listed)
    assert not missing, "included by the HIP sources but not hashed by mdbn_amd/build.py: %s" % missing


def test_source_hash_follows_every_build_input(tmp_path, monkeypatch):
    from mdbn_amd import build
    csrc = tmp_path / "mdbn_amd" / "csrc"
    shutil.copytree(build.CSRC, csrc, ignore=shutil.ignore_patterns(".obj"))
    (tmp_path / "include").mkdir()
    shutil.copy(HEADER, tmp_path / "include" / "mdbn_hip.h")
    monkeypatch.setattr(build, "CSRC", str(csrc))
    base = build.source_hash()
    for f in sorted(_includes_reachable(str(csrc), build.SOURCES)):
        p = os.path.join(str(csrc), f)
        old = open(p, "rb").read()
        with open(p, "ab") as fh:
            fh.write(b"\n// edited\n")
        assert build.source_hash() != base, "editing %s leaves source_hash() unchanged: a stale library would be kept" % f
        with open(p, "wb") as fh:
            fh.write(old)
        assert build.source_hash() == base, f


@pytest.mark.parametrize("name", sorted(KNOBS))
def test_refused_values_are_refused_by_a_range_check(name):
    """Every listed invalid value of a knob meets a check in its mdbn_set_option branch (the GPU test runs them through
    the library: test_gpu_knobs.py::test_refused_values_keep_the_previous_setting); a knob with no check takes any value
    as a flag (value != 0)."""
    body = _set_option_body()
    at = body.index('strcmp(name, "%s")' % name)
    branch = body[at:body.index("return MDBN_OK;", at)]
    if KNOBS[name]["invalid"]:
        assert "REQUIRE(" in branch or "fail(MDBN_EINVAL" in branch, name
    else:
        assert re.search(r"= value != 0;", branch), "%s takes integers but lists no invalid value" % name
