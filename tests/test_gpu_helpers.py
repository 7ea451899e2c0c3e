"""The helper kernels at the end of csrc/mdbn_kernels.hip -- round_flip, pl_cost, recon_cost, tanh, count_nonfinite, the bf16
wire conversions, the two gathers -- at edge values and at the launch geometries where such kernels go wrong: the body/tail
switch of the 8-wide bf16 kernels, the second pass of a grid-stride loop, `i % ld` against `i % cols`, an atomic across
waves, the pad columns.  The references are those of tests/_helpers_np.py (pinned on the CPU by tests/test_helpers_twin.py).

The C ABI is called directly (hip_engine.lib) where the engine's wrapper would hide the argument under test: `ld`, the
workspace, a preset `count`, `workgroups` / `threads`.  A buffer whose pad columns or tail must stay untouched is allocated
here with a recognisable fill -- outputs 7.0f (bf16: 0x7F7F), input pads NaN -- and the fill is checked afterwards."""
import ctypes as C

import numpy as np
import pytest

import _helpers_np as R
from _margins import check
from oracle import rbm_np
from test_gpu_saturated import _bound, _ladder_matrix, _pl_twin

pytestmark = pytest.mark.gpu

EINVAL = -1
SIGN = np.uint32(0x80000000)


# ------------------------------------------------------------------ plumbing

def _dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _ok(eng, rc, what):
    from mdbn_amd import _lib
    _lib.check(rc, what)


def _host_bits(t):
    """A float32 device tensor as uint32 patterns on the host."""
    import torch
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _padded(live, ld, fill):
    """[rows, ld] float32 with `live` in the leading columns and `fill` in the pad."""
    buf = np.full((live.shape[0], ld), fill, dtype=np.float32)
    buf[:, :live.shape[1]] = live
    return buf


def _patterns(bits):
    return sorted({"0x%08X" % b for b in np.asarray(bits).ravel().tolist()})


# ------------------------------------------------------------------ 2. round_flip

ROUND_SHAPES = [(1, 1, 4), (5, 7, 8), (37, 130, 132), (3, 255, 260), (64, 33, 64)]
GUARD = 64


@pytest.mark.parametrize("rows,cols,ld", ROUND_SHAPES)
def test_round_flip_is_bit_exact_on_the_edge_list(hip_engine, rows, cols, ld):
    """out = tensor.round(x), column flip_col = 1 - that, against round_half_away in float64 cast to float32: the edge list
    with both signs laid out cyclically, NaN in the input pads, sevens behind the output."""
    import torch
    eng = hip_engine
    x = R.cyclic(R.round_edges(), rows, cols)
    xin = _padded(x, ld, np.nan)
    want = R.round_half_away(x.astype(np.float64)).astype(np.float32)
    d_x = _dev(eng, xin)
    for flip in sorted({-1, 0, cols - 1}):
        out = torch.full((rows * ld + GUARD,), 7.0, dtype=torch.float32, device=eng.device)
        _ok(eng, eng.lib.mdbn_round_flip(eng.ctx, eng._stream(), _p(d_x), rows, cols, ld, flip, _p(out)), "mdbn_round_flip")
        w = want.copy()
        if flip >= 0:
            w[:, flip] = np.float32(1) - w[:, flip]
        got = _host_bits(out)
        body, tail = got[:rows * ld].reshape(rows, ld), got[rows * ld:]
        live = body[:, :cols]
        nan = np.isnan(w)
        assert np.isnan(live.view(np.float32)[nan]).all(), "NaN did not stay NaN (flip_col %d)" % flip
        bad = (live != R.bits32(w).reshape(rows, cols)) & ~nan
        assert not bad.any(), "flip_col %d: %d wrong, inputs %s -> got %s, want %s" % (
            flip, int(bad.sum()), _patterns(R.bits32(x).reshape(rows, cols)[bad])[:8], _patterns(live[bad])[:8],
            _patterns(R.bits32(w).reshape(rows, cols)[bad])[:8])
        zero = (w == 0) & ~nan                                  # (bit equality above already covers it; said on its own)
        assert ((live[zero] >> 31) == np.signbit(w[zero])).all(), "sign of a zero result"
        assert not body[:, cols:].any(), "pad columns of out are not +0"
        assert (tail == R.bits32(np.float32(7.0))).all(), "written behind the last row"
    np.testing.assert_array_equal(_host_bits(d_x), R.bits32(xin), "the input changed")


def test_pseudo_likelihood_cost_with_a_column_just_below_one_half(hip_engine):
    """RBM.get_pseudo_likelihood_cost on a 12 -> 7 layer, 8 rows, every entry of column bit_i_idx 0.49999997 (0x3EFFFFFF): it
    rounds to 0 and flips to 1.  A kernel that rounds it to 1 swaps the two free energies, and the cost is off by the whole
    difference.  Tolerance of test_monitoring_costs_on_device."""
    import mdbn_amd
    V, H, B = 12, 7, 8
    rs = np.random.RandomState(2)
    rbm = mdbn_amd.RBM(n_visible=V, n_hidden=H, numpy_rng=np.random.RandomState(9), engine=hip_engine)
    rbm.hbias.set_value(rs.normal(0, 0.5, H).astype(np.float32))
    rbm.vbias.set_value(rs.normal(0, 0.5, V).astype(np.float32))
    st = rbm_np.RBMState(V, H, W=rbm.W.get_value(), hbias=rbm.hbias.get_value(), vbias=rbm.vbias.get_value())
    x = (rs.uniform(size=(B, V)) < 0.5).astype(np.float32)
    for i in (0, 1, 2):
        assert rbm.bit_i_idx == i
        xi = x.copy()
        xi[:, i] = R.f32([R.BELOW_HALF])[0]
        st.bit_i_idx = i
        got = rbm.get_pseudo_likelihood_cost(xi)
        want = rbm_np.pseudo_likelihood_cost(st, xi.astype(np.float64))
        xw = xi.astype(np.float64); xw[:, i] = 1.0             # what a round to 1 would score: the regression is visible
        wrong = rbm_np.pseudo_likelihood_cost(st, xw)
        assert abs(wrong - want) > 100 * (1e-4 * abs(want) + 1e-6)
        print("PL with column %d at 0x3EFFFFFF: %.6f, float64 %.6f (rounded to 1 it would be %.6f)" % (i, got, want, wrong))
        assert abs(got - want) <= 1e-4 * abs(want) + 1e-6, (i, got, want, wrong)


# ------------------------------------------------------------------ 3. pl_cost / recon_cost: launch geometry

@pytest.mark.parametrize("rows", [1, 63, 64, 255, 256, 257, 5000])
def test_pl_cost_row_counts_around_the_workgroup(hip_engine, rows):
    """One workgroup of 256 threads strides over the rows: fewer rows than a wave, a wave, a workgroup +- 1, twenty passes.
    Inputs and bound of test_pl_cost_of_differences_on_the_ladder."""
    V = 130
    rs = np.random.RandomState(100 + rows)
    fe = rs.normal(0, 2000, rows).astype(np.float32)
    fe_flip = (fe - _ladder_matrix(rs, 1, rows)[0]).astype(np.float32)
    got = float(hip_engine.pl_cost(hip_engine.to_device(fe), hip_engine.to_device(fe_flip), V))
    want, w32 = _pl_twin(fe, fe_flip, V, False), _pl_twin(fe, fe_flip, V, True)
    gap = abs(w32 - want)
    bound = _bound(gap, 1e-4 * abs(want) + 1e-6)
    print("pl_cost %d rows: %.6f, float64 %.6f, gap of the restatement %.3e, bound %.3e, device %.3e"
          % (rows, got, want, gap, bound, abs(got - want)))
    assert np.isfinite(got)
    check("helpers pl_cost %d rows: abs" % rows, abs(got - want), bound)


RECON_SHAPES = [(1, 1), (1, 255), (1, 257), (37, 130), (513, 3), (700, 500)]     # the last: 1024 workgroups, a second pass


@pytest.mark.parametrize("wide", ["target", "pre"])
@pytest.mark.parametrize("gauss", [False, True], ids=["rbm", "grbm"])
@pytest.mark.parametrize("rows,cols", RECON_SHAPES)
def test_recon_cost_strides_and_grid(hip_engine, rows, cols, gauss, wide):
    """mdbn_recon_cost with ld_pre != ld_target (either the wider one), NaN in both pads and a workspace of exactly 4096
    bytes in front of a guard, on pre = ladder +- U(0, 1): relative 2e-6 against the float64 oracle.

    Element (0, 0) of the Bernoulli target is put on the wrong side of its pre-activation: a cost of e^-120, which the
    one-element case would otherwise have, lies below float32's smallest subnormal and has no relative bound in float32."""
    import torch
    eng = hip_engine
    rs = np.random.RandomState(7 * rows + cols)
    pre = _ladder_matrix(rs, rows, cols)
    if gauss:
        d = rs.uniform(0.1, 1, (rows, cols)) * rs.choice([-1.0, 1.0], (rows, cols))
        tgt = (rbm_np.sigmoid(pre.astype(np.float64)) + d).astype(np.float32)
    else:
        tgt = (rs.uniform(size=(rows, cols)) < 0.5).astype(np.float32)
        tgt[0, 0] = 1.0 if pre[0, 0] < 0 else 0.0
    ld = R.round_up4(cols)
    ld_pre, ld_tgt = (ld, ld + 8) if wide == "target" else (ld + 8, ld)
    d_pre, d_tgt = _dev(eng, _padded(pre, ld_pre, np.nan)), _dev(eng, _padded(tgt, ld_tgt, np.nan))
    ws = torch.full((1024 + GUARD,), 7.0, dtype=torch.float32, device=eng.device)
    out = torch.full((1 + GUARD,), 7.0, dtype=torch.float32, device=eng.device)
    _ok(eng, eng.lib.mdbn_recon_cost(eng.ctx, eng._stream(), _p(d_pre), ld_pre, _p(d_tgt), ld_tgt, rows, cols, int(gauss),
                                     _p(out), _p(ws), 4096), "mdbn_recon_cost")
    out, ws = out.cpu().numpy(), ws.cpu().numpy()
    assert (ws[1024:] == 7.0).all(), "written behind the 4096-byte workspace"
    assert (out[1:] == 7.0).all(), "written behind cost_out"
    got = float(out[0])
    want = float(rbm_np.reconstruction_cost(rbm_np.RBMState(1, 1, gauss=gauss), pre.astype(np.float64), tgt.astype(np.float64)))
    rel = abs(got - want) / abs(want)
    print("recon_cost %s %dx%d ld_pre %d ld_target %d: %.7g, float64 %.7g, rel %.3e"
          % ("GRBM" if gauss else "RBM", rows, cols, ld_pre, ld_tgt, got, want, rel))
    assert np.isfinite(got)
    check("helpers recon_cost %s %dx%d: rel" % ("GRBM" if gauss else "RBM", rows, cols), rel, 2e-6)


# ------------------------------------------------------------------ 4. the bf16 wire conversions

def _narrow(eng, u, src_offset=0):
    """mdbn_f32_to_bf16 of the patterns u into a destination with 16 guard elements: (rc, uint16 [n + 16])."""
    import torch
    n = len(u)
    src = _dev(eng, np.concatenate([u, np.zeros(8, np.uint32)]).view(np.int32))
    dst = torch.full((n + 16,), R.BF16_GUARD, dtype=torch.int16, device=eng.device)
    rc = eng.lib.mdbn_f32_to_bf16(eng.ctx, eng._stream(), _p(src, src_offset), _p(dst), n)
    return rc, dst.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("n", R.BF16_LENGTHS)
def test_f32_to_bf16_is_round_to_nearest_even_bit_for_bit(hip_engine, n):
    cases = R.bf16_cases()
    u = cases[np.arange(n) % len(cases)]
    rc, got = _narrow(hip_engine, u)
    _ok(hip_engine, rc, "mdbn_f32_to_bf16")
    assert (got[n:] == R.BF16_GUARD).all(), "written behind element n = %d" % n
    want, nan = R.bf16_rne_bits(u), R.is_nan_f32_bits(u)
    assert R.is_nan_bf16(got[:n][nan]).all(), "a NaN did not stay a NaN"
    assert ((got[:n][nan] >> 15) == (u[nan] >> 31)).all(), "a NaN lost its sign"
    bad = (got[:n] != want) & ~nan
    assert not bad.any(), "n = %d: %d wrong at %s, inputs %s" % (n, int(bad.sum()), np.flatnonzero(bad)[:8].tolist(),
                                                                _patterns(u[bad])[:8])


def test_f32_to_bf16_of_subnormal_inputs(hip_engine, capsys):
    """The header promises round-to-nearest-even; a conversion that flushes a subnormal input to a zero of its sign is the one
    other outcome allowed.  Which one it was is printed (and stated above mdbn_f32_to_bf16 in include/mdbn_hip.h: on the
    MI355X all eight were rounded to nearest even, none flushed)."""
    u = np.concatenate([R.BF16_SUBNORMAL_BITS, R.BF16_SUBNORMAL_BITS | SIGN])
    rc, got = _narrow(hip_engine, u)
    _ok(hip_engine, rc, "mdbn_f32_to_bf16")
    got, rne, zero = got[:len(u)], R.bf16_rne_bits(u), (u >> 16).astype(np.uint16) & 0x8000
    outcome = ["RNE" if g == r else "flushed" if g == z else "0x%04X" % g for g, r, z in zip(got, rne, zero)]
    with capsys.disabled():
        print("\nf32 -> bf16 of subnormal inputs: " + ", ".join("0x%08X -> 0x%04X (%s)" % (a, g, o) for a, g, o in zip(u, got, outcome)))
    assert all(o in ("RNE", "flushed") for o in outcome), outcome
    assert ((got >> 15) == (u >> 31)).all()


def test_bf16_to_f32_of_every_pattern(hip_engine):
    import torch
    eng = hip_engine
    pat = np.arange(65536, dtype=np.uint32)
    src = _dev(eng, pat.astype(np.uint16).view(np.int16))
    dst = torch.full((65536 + 16,), 7.0, dtype=torch.float32, device=eng.device)
    _ok(eng, eng.lib.mdbn_bf16_to_f32(eng.ctx, eng._stream(), _p(src), _p(dst), 65536), "mdbn_bf16_to_f32")
    got = _host_bits(dst)
    np.testing.assert_array_equal(got[:65536], pat << 16)                          # NaN payloads included
    assert (got[65536:] == R.bits32(np.float32(7.0))).all()


@pytest.mark.parametrize("n", R.BF16_LENGTHS)
def test_bf16_to_f32_lengths(hip_engine, n):
    import torch
    eng = hip_engine
    pat = ((np.arange(n, dtype=np.uint32) * 40503 + 0x3F7F) & 0xFFFF).astype(np.uint16)       # a walk over all patterns
    src = _dev(eng, np.concatenate([pat, np.zeros(8, np.uint16)]).view(np.int16))
    dst = torch.full((n + 16,), 7.0, dtype=torch.float32, device=eng.device)
    _ok(eng, eng.lib.mdbn_bf16_to_f32(eng.ctx, eng._stream(), _p(src), _p(dst), n), "mdbn_bf16_to_f32")
    got = _host_bits(dst)
    np.testing.assert_array_equal(got[:n], pat.astype(np.uint32) << 16)
    assert (got[n:] == R.bits32(np.float32(7.0))).all(), "written behind element n = %d" % n


def test_bf16_conversions_refuse_a_misaligned_base(hip_engine):
    import torch
    eng = hip_engine
    rc, got = _narrow(eng, R.bf16_cases()[:64], src_offset=4)
    assert rc == EINVAL and (got == R.BF16_GUARD).all()
    f = torch.full((80,), 7.0, dtype=torch.float32, device=eng.device)
    h = torch.full((96,), R.BF16_GUARD, dtype=torch.int16, device=eng.device)
    assert eng.lib.mdbn_f32_to_bf16(eng.ctx, eng._stream(), _p(f), _p(h, 4), 64) == EINVAL
    assert eng.lib.mdbn_bf16_to_f32(eng.ctx, eng._stream(), _p(h, 4), _p(f), 64) == EINVAL
    assert eng.lib.mdbn_bf16_to_f32(eng.ctx, eng._stream(), _p(h), _p(f, 4), 64) == EINVAL
    assert bool((f == 7.0).all()) and bool((h == R.BF16_GUARD).all())


# ------------------------------------------------------------------ 5. count_nonfinite

BAD = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA00000, 0xFFC00001], dtype=np.uint32)    # +-inf, quiet / signalling NaN
FINE = np.array([0x7F7FFFFF, 0x80000000, 0x00000123, 0xFF7FFFFF], dtype=np.uint32)     # FLT_MAX, -0, a subnormal, -FLT_MAX


def _count(eng, u, preset, n=None):
    x = _dev(eng, np.asarray(u, dtype=np.uint32).view(np.int32))
    count = _dev(eng, np.array([preset, 7, 7, 7], dtype=np.int32))
    _ok(eng, eng.lib.mdbn_count_nonfinite(eng.ctx, eng._stream(), _p(x), len(u) if n is None else n, _p(count)),
        "mdbn_count_nonfinite")
    count = count.cpu().numpy()
    assert (count[1:] == 7).all()
    return int(count[0])


def test_count_nonfinite_over_a_full_grid_and_a_second_pass(hip_engine):
    n = 2048 * 256 + 300
    u = np.zeros(n, dtype=np.uint32)
    where = [0, 63, 64, 255, 256, 524287, 524288, n - 1]
    for k, i in enumerate(where):
        u[i] = BAD[k % len(BAD)]
    for k, i in enumerate([1, 62, 65, 254, 257, 524286, 524289, n - 2]):             # finite neighbours that must not count
        u[i] = FINE[k % len(FINE)]
    assert _count(hip_engine, u, preset=5) == 5 + len(where) == 13


def test_count_nonfinite_small_cases(hip_engine):
    eng = hip_engine
    assert _count(eng, BAD, preset=5, n=0) == 5                                      # n = 0 leaves count alone
    for b in BAD:
        assert _count(eng, [b], preset=0) == 1
    assert _count(eng, FINE, preset=0) == 0
    # every wave all bad, the atomic hit by every wave of 274 workgroups
    assert _count(eng, np.full(70000, 0x7FC00000, dtype=np.uint32), preset=0) == 70000


def test_count_nonfinite_through_the_engine_scans_the_pad(hip_engine):
    t = hip_engine.alloc_matrix(5, 6)
    assert t._base.shape[1] > 6
    assert hip_engine.count_nonfinite(t) == 0
    t._base[2, 7] = float("nan")
    assert hip_engine.count_nonfinite(t) == 1                                        # "the whole storage"
    t[4, 0] = float("inf")
    assert hip_engine.count_nonfinite(t, t) == 4


# ------------------------------------------------------------------ 6. tanh

# For |x| < 2^-10 the absolute bound says nothing (tanh x = x (1 - x^2 / 3 ..): a near-identity).  Worst relative error against
# float64 measured on the MI355X over the 64 such arguments of each layout: 3.302e-8 (at x = 3.147e-4; below 2^-24 = 5.96e-8,
# the rounding of the result alone).  Asserted at 4x that; the cap would have been 2^-20 = 9.5e-7 (three lost bits).
TANH_SMALL_REL = 4 * 3.302e-8
assert TANH_SMALL_REL <= 2.0 ** -20


@pytest.mark.parametrize("rows,cols,ld", [(9, 21, 24), (3, 257, 320)])
def test_tanh_values_layout_and_oddness(hip_engine, rows, cols, ld):
    import torch
    eng = hip_engine
    x, h = R.tanh_values(rows * cols, seed=cols)
    buf = _dev(eng, np.concatenate([_padded(x.reshape(rows, cols), ld, 7.0).ravel(), np.full(GUARD, 7.0, np.float32)]))
    _ok(eng, eng.lib.mdbn_tanh(eng.ctx, eng._stream(), _p(buf), rows, cols, ld), "mdbn_tanh")
    got = buf.cpu().numpy()
    body = got[:rows * ld].reshape(rows, ld)
    assert (body[:, cols:] == 7.0).all() and (got[rows * ld:] == 7.0).all(), "pad columns or the tail were written"
    out = np.ascontiguousarray(body[:, :cols]).ravel()
    want = np.tanh(x.astype(np.float64))
    nan = np.isnan(x)
    assert nan.sum() == 1 and np.isnan(out[nan]).all() and not np.isnan(out[~nan]).any()
    assert np.abs(out[~nan]).max() <= 1.0
    inf = np.isinf(x)
    assert inf.sum() == 2 and np.array_equal(out[inf], np.sign(x[inf]))
    check("helpers tanh %dx%d: abs" % (rows, cols), np.abs(out[~nan] - want[~nan]).max(), 2e-6)
    np.testing.assert_array_equal(R.bits32(out[h:2 * h]), R.bits32(out[:h]) ^ SIGN, "tanh(-x) != -tanh(x) bit for bit")
    small = (np.abs(x) < R.TANH_SMALL) & (x != 0) & ~nan
    assert small.sum() >= 60
    rel = np.abs(out[small] - want[small]) / np.abs(want[small])
    print("tanh %dx%d: worst relative error over %d arguments below 2^-10: %.3e (at x = %r)"
          % (rows, cols, int(small.sum()), rel.max(), float(x[small][rel.argmax()])))
    check("helpers tanh small-argument: rel", rel.max(), TANH_SMALL_REL)


# ------------------------------------------------------------------ 7. the gathers

N_ROWS, N_IDX = 50, 37


def _gather_problem(cols, wide):
    rs = np.random.RandomState(cols)
    ld = R.round_up4(cols)
    ld_src, ld_dst = (ld + 8, ld) if wide == "src" else (ld, ld + 8)
    src = _padded(rs.normal(size=(N_ROWS, cols)).astype(np.float32), ld_src, 0.0)        # zero pads: the layout contract
    idx = rs.randint(-N_ROWS, N_ROWS, N_IDX)
    idx[:6] = [-1, -50, 49, 0, 17, 17]                                               # both ends, either way; duplicates
    idx[-1] = idx[7]
    assert idx.min() >= -N_ROWS and idx.max() < N_ROWS and len(set(idx.tolist())) < N_IDX
    return src, idx, ld, ld_src, ld_dst


def _check_gather(tag, dst, n, src, rows, cols, ld, ld_dst):
    dst = dst.cpu().numpy()
    body, tail = dst[:n * ld_dst].reshape(n, ld_dst), dst[n * ld_dst:]
    np.testing.assert_array_equal(R.bits32(body[:, :cols]), R.bits32(src[rows, :cols]), tag)
    assert not R.bits32(body[:, cols:ld]).any(), "%s: the pad up to round_up4(cols) is the source's zero pad" % tag
    assert (body[:, ld:] == 7.0).all(), "%s: columns beyond round_up4(cols) were written" % tag
    assert (tail == 7.0).all(), "%s: rows behind the last one were written" % tag


def _index_lists(eng, idx):
    """(label, device index tensor or None, index_is_64, n_idx, the rows it names)"""
    for dt in (np.int32, np.int64):
        yield np.dtype(dt).name, _dev(eng, idx.astype(dt)), int(dt == np.int64), N_IDX, idx % N_ROWS
    yield "identity", None, 0, N_ROWS, np.arange(N_ROWS)


@pytest.mark.parametrize("wide", ["src", "dst"])
@pytest.mark.parametrize("cols", [5, 130, 1036])
def test_gather_rows_strides_duplicates_and_negative_indexes(hip_engine, cols, wide):
    import torch
    eng = hip_engine
    src, idx, ld, ld_src, ld_dst = _gather_problem(cols, wide)
    d_src = _dev(eng, src)
    for label, d_idx, is64, n, rows in _index_lists(eng, idx):
        dst = torch.full((n * ld_dst + 2 * ld_dst,), 7.0, dtype=torch.float32, device=eng.device)
        _ok(eng, eng.lib.mdbn_gather_rows(eng.ctx, eng._stream(), _p(d_src), N_ROWS, cols, ld_src,
                                          None if d_idx is None else _p(d_idx), is64, n, _p(dst), ld_dst), "mdbn_gather_rows")
        _check_gather("gather %s" % label, dst, n, src, rows, cols, ld, ld_dst)


@pytest.mark.parametrize("wide", ["src", "dst"])
@pytest.mark.parametrize("cols", [5, 130, 1036])
def test_gather_rows_host_launch_geometries(hip_engine, cols, wide):
    """The slim kernel from pinned host memory: one workgroup of 64 threads (cols = 1036: two column passes, the second one
    partial), the defaults, more workgroups than rows, a row stride of 7."""
    import torch
    eng = hip_engine
    src, idx, ld, ld_src, ld_dst = _gather_problem(cols, wide)
    host = torch.from_numpy(src).pin_memory()
    for label, d_idx, is64, n, rows in _index_lists(eng, idx):
        for wg, threads in ((1, 64), (0, 0), (1024, 128), (7, 256)):
            dst = torch.full((n * ld_dst + 2 * ld_dst,), 7.0, dtype=torch.float32, device=eng.device)
            _ok(eng, eng.lib.mdbn_gather_rows_host(eng.ctx, eng._stream(), _p(host), N_ROWS, cols, ld_src,
                                                   None if d_idx is None else _p(d_idx), is64, n, _p(dst), ld_dst, wg, threads),
                "mdbn_gather_rows_host")
            _check_gather("host gather %s %d x %d" % (label, wg, threads), dst, n, src, rows, cols, ld, ld_dst)


def test_gather_rows_host_refuses_bad_launch_geometry(hip_engine):
    import torch
    eng = hip_engine
    src, idx, ld, ld_src, ld_dst = _gather_problem(5, "dst")
    host = torch.from_numpy(src).pin_memory()
    d_idx = _dev(eng, idx.astype(np.int32))
    dst = torch.full((N_IDX * ld_dst,), 7.0, dtype=torch.float32, device=eng.device)
    for wg, threads in ((32, 96), (1025, 256), (-1, 64)):
        rc = eng.lib.mdbn_gather_rows_host(eng.ctx, eng._stream(), _p(host), N_ROWS, 5, ld_src, _p(d_idx), 0, N_IDX, _p(dst),
                                           ld_dst, wg, threads)
        assert rc == EINVAL, (wg, threads, rc)
    assert bool((dst == 7.0).all())
