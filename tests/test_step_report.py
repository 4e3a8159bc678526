"""The step report (``dr_step_report``, ``densereg_amd/csrc/step_report.h``): per trainable variable, statistics of the weights, of
the averaged and clipped gradient and of the decrement the next ``dr_apply_adam`` would apply, without taking that step.

The reference of every test is ``restate`` below: ``adam_kernel``'s arithmetic in numpy fp32, one correctly rounded op per op of the
kernel (``fmaxf`` / ``fminf`` on a NaN written out).  ``test_it_is_the_step_apply_adam_takes`` ties that restatement to the engine's
own step bit for bit.  Bars: every count, histogram, min / max, ``raw_stats[:, 0]``, ``global[4:6]`` and ``global_counts`` EXACT (each
is an order-free function of per-element values); sums of squares and the norms at ``rtol = 2.5e-7`` (fp32 casts of fp64 sums of
non-negative terms); signed sums within ``2^-23 |ref| + 1e-9 sum|x_i|`` (the cast, and a generous multiple of the fp64
re-association bound ``n 2^-53 sum|x_i|`` = 6.5e-11 ``sum|x_i|`` at n = 589 824).  ``[emu]`` on the host-fiber emulator, ``[gpu]`` on
the MI355X.
"""
import ctypes as C
import functools
import io
import math
import types

import numpy as np
import pytest

from densereg_amd import _lib
from tests.common import _flat_rw

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def be(request):
    return request.getfixturevalue(request.param)


FIELDS = tuple(_lib.STEP_REPORT_FIELDS)
HISTS = ('grad_hist', 'param_hist')
SENT = -777                                         # no statistic of the test data and no count can take it
GUARD = 24
RTOL = 2.5e-7
NET = (1, 8, 3, 128)                                # S, F, J, in_hw: V = 229 variables, 1 867 521 elements
LR, DIV, CLIP, STEP = 1e-3, 5.0, 0.2, 7
INVALID, STATE = -1, -3


def _cfg():
    from oracle.graph import NetConfig
    return NetConfig(NET[0], NET[1], NET[2], in_hw=NET[3])


@functools.lru_cache(maxsize=None)
def _layout():
    """names, sizes, offsets of the trainable variables in flat order (oracle.graph.param_specs)"""
    from oracle.graph import param_specs
    names = [n for n, _, tr in param_specs(_cfg()) if tr]
    sizes = np.array([int(np.prod(s)) for _, s, tr in param_specs(_cfg()) if tr], np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    assert len(names) == 229 and sizes.sum() == 1867521
    assert {3, 4, 5, 7, 9, 55, 262144, 263680, 589824} <= set(sizes.tolist())
    return names, sizes, off


@functools.lru_cache(maxsize=None)
def _data():
    """acc, theta, m, v (float32, read-only): |acc| spread over 1e-9 ... 10 (div = 5, clip = 0.2: both sides of the clip in every
    large variable), one variable all zero, NaN / +Inf / -Inf at the first element of a variable, the last element of the flat buffer
    and inside the 589 824-element variable."""
    _, sizes, off = _layout()
    n = int(sizes.sum())
    rng = np.random.default_rng(20240)
    acc = (10.0 ** rng.uniform(-9, 1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    zero_var = int(np.nonzero((sizes > 500) & (sizes < 5000))[0][0])
    acc[off[zero_var]:off[zero_var] + sizes[zero_var]] = 0.0
    big = int(np.nonzero(sizes == 589824)[0][0])
    first = int(np.nonzero(sizes == 263680)[0][0])
    acc[off[first]] = np.nan
    acc[n - 1] = np.inf
    acc[off[big] + 300001] = -np.inf
    acc[off[big] + 4097] = np.nan
    acc[off[big] + 123457] = np.inf
    theta = (rng.standard_normal(n) * 0.1).astype(np.float32)
    m = (rng.standard_normal(n) * 0.05).astype(np.float32)
    v = (rng.uniform(0, 1, n) ** 4 * 0.01).astype(np.float32)
    v[rng.integers(0, n, 1000)] = 0.0
    for a in (acc, theta, m, v):
        a.setflags(write=False)
    return acc, theta, m, v


def lr_t_of(lr, step):
    """dr_apply_adam's bias-corrected step size: fp32 lr widened, fp64 arithmetic, one cast"""
    return np.float32(float(np.float32(lr)) * math.sqrt(1.0 - 0.999 ** float(step)) / (1.0 - 0.5 ** float(step)))


def restate(acc, theta, m, v, lr=LR, div=DIV, clip=CLIP, step=STEP):
    """adam_kernel op for op in fp32: a, g, m', v', u, theta'"""
    f = np.float32
    b1, b2, eps, lr_t = f(0.5), f(0.999), f(1e-8), lr_t_of(lr, step)
    with np.errstate(all='ignore'):
        a = acc / f(div)
        g = np.minimum(np.where(np.isnan(a), f(-clip), np.maximum(a, f(-clip))), f(clip))     # fminf(fmaxf(a, -clip), clip)
        m2 = b1 * m + (f(1.0) - b1) * g
        v2 = b2 * v + (f(1.0) - b2) * g * g
        u = lr_t * m2 / (np.sqrt(v2) + eps)
        th2 = theta - u
    for x in (a, g, m2, v2, u, th2):
        assert x.dtype == np.float32
    return a, g, m2, v2, u, th2


def _stats4(x, off):
    with np.errstate(all='ignore'):
        x64 = x.astype(np.float64)
        return np.stack([np.fmin.reduceat(x, off), np.fmax.reduceat(x, off), np.add.reduceat(x64, off),
                         np.add.reduceat(x64 * x64, off)], axis=1), np.add.reduceat(np.abs(x64), off)


def expected(acc, theta, m, v, edges=None, lr=LR, div=DIV, clip=CLIP, step=STEP):
    """every member in fp64 / int64, plus 'abs_<member>' = sum |x_i| per variable for the bar of the signed sums"""
    _, sizes, off = _layout()
    a, g, _, _, u, _ = restate(acc, theta, m, v, lr, div, clip, step)
    out = {}
    out['param_stats'], out['abs_param_stats'] = _stats4(theta, off)
    out['grad_stats'], out['abs_grad_stats'] = _stats4(g, off)
    out['update_stats'], out['abs_update_stats'] = _stats4(u, off)
    fin = np.isfinite(a)
    af = np.where(fin, a, np.float32(0)).astype(np.float64)
    out['raw_stats'] = np.stack([np.maximum.reduceat(np.abs(af), off), np.add.reduceat(af * af, off)], axis=1)
    cnt = lambda mask: np.add.reduceat(mask.astype(np.int64), off)
    out['grad_counts'] = np.stack([sizes, cnt(~np.isfinite(acc)), cnt(fin & (np.abs(a) > np.float32(clip))), cnt(acc == 0)], axis=1)
    out['global'] = np.array([math.sqrt(out['grad_stats'][:, 3].sum()), math.sqrt(out['raw_stats'][:, 1].sum()),
                              math.sqrt(out['param_stats'][:, 3].sum()), math.sqrt(out['update_stats'][:, 3].sum()),
                              np.abs(g).max(), np.abs(u).max()])
    out['global_counts'] = out['grad_counts'][:, 1:].sum(axis=0)
    if edges is not None:
        var = np.repeat(np.arange(len(sizes)), sizes)
        nb = len(edges) + 1
        for name, x in (('grad_hist', g), ('param_hist', theta)):
            b = np.searchsorted(edges, x, side='right')
            out[name] = np.bincount(var * nb + b, minlength=len(sizes) * nb).reshape(len(sizes), nb)
    return out


def _signed_ok(got, ref, sum_abs, what):
    err = np.abs(got.astype(np.float64) - ref)
    bar = 2.0 ** -23 * np.abs(ref) + 1e-9 * sum_abs
    print('%s: worst signed-sum error / bar %.3g' % (what, np.max(err / np.maximum(bar, 1e-300))))
    assert (err <= bar).all(), what


def check(got, exp, what=''):
    """the bars of the module docstring, member by member, for the members `got` holds"""
    for n in ('param_stats', 'grad_stats', 'update_stats'):
        if n in got:
            np.testing.assert_array_equal(got[n][:, :2], exp[n][:, :2].astype(np.float32), err_msg='%s %s min / max' % (what, n))
            _signed_ok(got[n][:, 2], exp[n][:, 2], exp['abs_' + n], '%s %s' % (what, n))
            np.testing.assert_allclose(got[n][:, 3], exp[n][:, 3].astype(np.float32), rtol=RTOL, atol=0, err_msg='%s %s' % (what, n))
    if 'raw_stats' in got:
        np.testing.assert_array_equal(got['raw_stats'][:, 0], exp['raw_stats'][:, 0].astype(np.float32), err_msg=what)
        np.testing.assert_allclose(got['raw_stats'][:, 1], exp['raw_stats'][:, 1].astype(np.float32), rtol=RTOL, atol=0, err_msg=what)
    if 'global' in got:
        rel = np.abs(got['global'][:4].astype(np.float64) / exp['global'][:4] - 1.0)
        print('%s global norms: relative deviation %s' % (what, rel))
        np.testing.assert_allclose(got['global'][:4], exp['global'][:4].astype(np.float32), rtol=RTOL, atol=0, err_msg=what)
        np.testing.assert_array_equal(got['global'][4:], exp['global'][4:].astype(np.float32), err_msg=what)
    for n in ('grad_counts', 'global_counts') + HISTS:
        if n in got and n in exp:
            np.testing.assert_array_equal(got[n], exp[n], err_msg='%s %s' % (what, n))


# ---- the handle -----------------------------------------------------------------------------------------------------
def _adam_addr(h):
    m, v, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    h.call('dr_flat_adam', C.byref(m), C.byref(v), C.byref(n))
    return m.value, v.value, n.value


class Flat:
    """read / write access to the handle's flat gradient, parameter and Adam moment buffers"""

    def __init__(self, be, h):
        gp, n = h.flat('grad')
        pp, n2 = h.flat('param')
        mp, vp, n3 = _adam_addr(h)
        assert n == n2 == n3
        self.n = n
        self.rw = {k: _flat_rw(be, p, n) for k, p in (('grad', gp), ('param', pp), ('m', mp), ('v', vp))}

    def write(self, **kw):
        for k, a in kw.items():
            self.rw[k][1](np.array(a, np.float32))

    def read(self, k):
        return np.array(self.rw[k][0]())


def _new_handle(be, B=2, fill=True):
    h = be.handle(_cfg(), B, training=True)
    fl = Flat(be, h)
    assert fl.n == int(_layout()[1].sum())
    if fill:
        acc, theta, m, v = _data()
        fl.write(grad=acc, param=theta, m=m, v=v)
    return h, fl


# The arithmetic tests only READ one handle per backend (no forward is needed, the report changes nothing): it is filled once.
_SHARED = {}


def _shared(be):
    if be.name not in _SHARED:
        _SHARED[be.name] = _new_handle(be)
    return _SHARED[be.name]


@pytest.fixture(scope='module', autouse=True)
def _close_shared_handles():
    yield
    for h, _ in _SHARED.values():
        h.close()
    _SHARED.clear()


def _shape(name, E):
    return tuple(_lib.STEP_REPORT_FIELDS[name][0](len(_layout()[0]), E))


class Buffers:
    """All nine output buffers, pre-filled with the sentinel and over-allocated by a guard tail"""

    def __init__(self, be, E):
        self.be, self.E = be, E
        self.dev = {}
        for n, (_, is_int) in _lib.STEP_REPORT_FIELDS.items():
            self.dev[n] = be.dev(np.full(int(np.prod(_shape(n, E))) + GUARD, SENT, np.int32 if is_int else np.float32))

    def struct(self, want, d_edges, E=None):
        rep = _lib.DrStepReport()
        rep.hist_edges_dev, rep.num_edges = self.be.ptr(d_edges), self.E if E is None else E
        for n in FIELDS:
            setattr(rep, n + '_dev', self.be.ptr(self.dev[n]) if n in want else None)
        return rep

    def read(self, want):
        """name -> payload of the requested members; they are fully written, guard tails and the other buffers untouched"""
        out = {}
        for n in FIELDS:
            a = np.array(self.be.host(self.dev[n]))
            payload, tail = a[:-GUARD].reshape(_shape(n, self.E)), a[-GUARD:]
            assert (tail == SENT).all(), '%s: guard tail written' % n
            if n in want:
                assert not (payload == SENT).any(), '%s: sentinel left in the payload' % n
                out[n] = payload
            else:
                assert (payload == SENT).all(), '%s: written although not requested' % n
        return out


def step_report(be, h, want=FIELDS, edges=None, lr=LR, div=DIV, clip=CLIP, step=STEP):
    E = 0 if edges is None else len(edges)
    d_edges = None if edges is None else be.dev(np.array(edges, np.float32))
    bufs = Buffers(be, E)
    rep = bufs.struct(want, d_edges)
    h.call('dr_step_report', C.c_float(lr), C.c_float(div), C.c_float(clip), C.c_int64(step), C.byref(rep), be.stream)
    be.sync()
    return bufs.read(want)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


EDGES5 = np.array([-1.0, -CLIP, 0.0, CLIP, 1.0], np.float32)


def _default_edges():
    from densereg_amd.engine import hist_edges
    return hist_edges()


# ---------------------------------------------------------------------------------------------
# 1. all members
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['default_edges', 'five_edges'])
def test_all_members(be, which):
    """Every member against the numpy restatement, with hist_edges() and with five edges that contain -clip, 0 and clip exactly:
    a value equal to an edge falls into the bucket to its right, so the bucket that starts at clip holds every clipped-high element
    (and the non-finite ones the clip maps there)."""
    edges = _default_edges() if which == 'default_edges' else EDGES5
    h, _ = _shared(be)
    acc, theta, m, v = _data()
    got = step_report(be, h, edges=edges)
    exp = expected(acc, theta, m, v, edges)
    check(got, exp, which)
    gc = got['grad_counts']
    assert gc[:, 1].sum() == 5 and (gc[:, 2] > 0).sum() > 50 and (gc[:, 3] == gc[:, 0]).sum() == 1      # the planted cases are there
    assert (got['grad_stats'][:, 3][gc[:, 3] == gc[:, 0]] == 0).all()
    if which == 'five_edges':
        a = acc / np.float32(DIV)
        hi = np.add.reduceat(((a >= np.float32(CLIP)) & ~np.isnan(a)).astype(np.int64), _layout()[2])
        np.testing.assert_array_equal(got['grad_hist'][:, 4], hi)       # g == clip exactly: bucket [clip, 1)
        assert (got['grad_hist'][:, 5] == 0).all() and (got['grad_hist'][:, 0] == 0).all()       # nothing beyond the clip
        assert got['grad_hist'].sum() == acc.size and got['param_hist'].sum() == acc.size


# ---------------------------------------------------------------------------------------------
# 2. member subsets, 3. determinism
# ---------------------------------------------------------------------------------------------
def test_report_is_deterministic_and_members_are_independent(be):
    """Two calls: the same bits in every member.  Each member alone and {global, global_counts}: the bits of the all-members call,
    nothing else written (checked against sentinels and guard tails inside step_report)."""
    h, _ = _shared(be)
    full = step_report(be, h, edges=EDGES5)
    again = step_report(be, h, edges=EDGES5)
    for n in FIELDS:
        np.testing.assert_array_equal(_bits(full[n]), _bits(again[n]), err_msg=n)
    for want in [(n,) for n in FIELDS] + [('global', 'global_counts')]:
        got = step_report(be, h, want=want, edges=EDGES5 if set(want) & set(HISTS) else None)
        assert set(got) == set(want)
        for n in want:
            np.testing.assert_array_equal(_bits(got[n]), _bits(full[n]), err_msg='%s in %s' % (n, want))
    # edges given although no histogram is wanted: allowed, and they change nothing
    got = step_report(be, h, want=('grad_stats',), edges=EDGES5)
    np.testing.assert_array_equal(_bits(got['grad_stats']), _bits(full['grad_stats']))


# ---------------------------------------------------------------------------------------------
# 4. it is the step dr_apply_adam takes
# ---------------------------------------------------------------------------------------------
def test_it_is_the_step_apply_adam_takes(be):
    """Report, then dr_apply_adam with the same arguments: m', v' and theta - u of the restatement are the engine's m, v and theta bit
    for bit (so the reference of every other test IS the step), and the report's sum u^2 per variable matches the restatement's."""
    h, fl = _new_handle(be)
    acc, theta, m, v = _data()
    got = step_report(be, h, want=('update_stats', 'global'))
    h.call('dr_apply_adam', C.c_float(LR), C.c_float(DIV), C.c_float(CLIP), C.c_int64(STEP), be.stream)
    be.sync()
    _, _, m2, v2, u, th2 = restate(acc, theta, m, v)
    e_m, e_v, e_th, e_g = fl.read('m'), fl.read('v'), fl.read('param'), fl.read('grad')
    h.close()
    np.testing.assert_array_equal(_bits(e_m), _bits(m2))
    np.testing.assert_array_equal(_bits(e_v), _bits(v2))
    np.testing.assert_array_equal(_bits(e_th), _bits(th2))
    np.testing.assert_array_equal(_bits(e_g), _bits(acc))                  # the report and the step leave the accumulator alone
    su2 = np.add.reduceat(u.astype(np.float64) ** 2, _layout()[2])
    np.testing.assert_allclose(got['update_stats'][:, 3], su2.astype(np.float32), rtol=RTOL, atol=0)
    np.testing.assert_allclose(got['global'][3], np.float32(math.sqrt(su2.sum())), rtol=RTOL, atol=0)


# ---------------------------------------------------------------------------------------------
# 5. read-only through a real step
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net_inputs(B):
    from densereg_amd.data.synthetic import make_crops
    from oracle import net as onet, pose
    cfg = _cfg()
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=5, hw=cfg.in_hw)
    poses = np.ascontiguousarray(poses[:, :3 * cfg.num_jnt])
    ndm = pose.norm_dm(dm, coms)
    params = onet.make_test_params(cfg, ndm[:4], seed=7)
    return params, (ndm, poses, cfgs, coms)


def _real_step(be, depth, with_reports):
    """zero_grad, two micro-steps (forward with DR_DROPOUT_RNG, loss, backward) of B = 2, dr_apply_adam; optionally a report of all
    members after each backward.  Returns theta, m, v, the flat gradient after the step, and the reports."""
    B = 2
    params, inputs = _net_inputs(B)
    h = be.handle(_cfg(), B, training=True)
    h.load_params(params)
    h.call('dr_finalize_params', be.stream)
    fl = Flat(be, h)
    rng = np.random.default_rng(3)
    fl.write(m=(rng.standard_normal(fl.n) * 1e-3).astype(np.float32), v=(rng.uniform(0, 1e-5, fl.n)).astype(np.float32))
    if depth == 2:
        h.call('dr_set_pipeline', 2)
    h.call('dr_zero_grad', be.stream)
    d_in = [be.dev(np.array(a, np.float32)) for a in inputs]
    reports = []
    for k in range(2):
        h.call('dr_forward_train', B, be.ptr(d_in[0]), _lib.DROPOUT_RNG, None, C.c_uint64(11 + k), be.stream)
        h.call('dr_loss', B, *[be.ptr(a) for a in d_in], None, be.stream)
        h.call('dr_backward', B, be.stream)
        if with_reports:
            reports.append(step_report(be, h, edges=EDGES5, div=2.0, step=1))
    h.call('dr_apply_adam', C.c_float(LR), C.c_float(2.0), C.c_float(CLIP), C.c_int64(1), be.stream)
    be.sync()
    out = {k: fl.read(k) for k in ('param', 'm', 'v', 'grad')}
    h.close()
    return out, reports


_STEP1 = {}


@pytest.mark.parametrize('depth', [1, 2])
def test_report_is_read_only_through_a_real_step(be, depth):
    """The same optimizer step from identical state with and without dr_step_report (all members) after each backward: parameters,
    m, v and the flat gradient have the same bits afterwards, at pipeline depth 1 and at depth 2 (where the report reads both slots'
    accumulators and folds neither).  The last report describes the step that was then taken: its update norm is the norm of
    theta_before - theta_after.  Depth 2 against depth 1: dr_set_pipeline promises the depth-1 result up to the rounding of one
    addition per element (the accumulators' bits differ, so no count is compared); for the norm of the raw gradient that is a few
    2^-24 relative as long as the two micro-steps' gradients do not cancel -- they are two dropout draws on the same crops --, held
    here at 1e-5."""
    plain, _ = _real_step(be, depth, False)
    rep, reports = _real_step(be, depth, True)
    for k in plain:
        np.testing.assert_array_equal(_bits(plain[k]), _bits(rep[k]), err_msg=k)
    last = reports[-1]
    assert last['global_counts'][0] == 0 and last['grad_counts'][:, 0].sum() == plain['param'].size
    # the gradient the report saw is the one the step applied: restate the step from the final accumulator
    theta0 = np.concatenate([_net_inputs(2)[0][n].reshape(-1) for n in _layout()[0]]).astype(np.float32)
    rng = np.random.default_rng(3)
    m0 = (rng.standard_normal(theta0.size) * 1e-3).astype(np.float32)
    v0 = (rng.uniform(0, 1e-5, theta0.size)).astype(np.float32)
    exp = expected(plain['grad'], theta0, m0, v0, EDGES5, div=2.0, step=1)
    check(last, exp, 'depth %d' % depth)
    np.testing.assert_array_equal(_bits(restate(plain['grad'], theta0, m0, v0, div=2.0, step=1)[5]), _bits(plain['param']))
    _STEP1[(be.name, depth)] = last
    if (be.name, 1) in _STEP1 and (be.name, 2) in _STEP1:
        a, b = _STEP1[(be.name, 1)]['global'], _STEP1[(be.name, 2)]['global']
        print('depth 1 / depth 2 global norms: %s / %s' % (a, b))
        np.testing.assert_allclose(a[:4], b[:4], rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------------------------
def test_error_contract(be):
    h, _ = _shared(be)
    lib = h.lib
    d_edges = be.dev(EDGES5)
    bufs = Buffers(be, len(EDGES5))
    good = bufs.struct(FIELDS, d_edges)

    def call(rep, lr=LR, div=DIV, clip=CLIP, step=STEP, handle=h._h):
        return lib.dr_step_report(handle, C.c_float(lr), C.c_float(div), C.c_float(clip), C.c_int64(step),
                                  None if rep is None else C.byref(rep), be.stream)
    assert call(good, handle=None) == INVALID
    assert call(None) == INVALID and b'NULL' in lib.dr_last_error(h._h)
    assert call(bufs.struct((), d_edges)) == INVALID                       # no output member
    for bad_step in (0, -3):
        assert call(good, step=bad_step) == INVALID
    for bad in (0.0, -1.0, float('nan')):
        assert call(good, div=bad) == INVALID
        assert call(good, clip=bad) == INVALID
    for bad_e in (-1, 2049):
        assert call(bufs.struct(FIELDS, d_edges, E=bad_e)) == INVALID
    for hist in HISTS:                                                       # a histogram without edges
        assert call(bufs.struct((hist,), None, E=0)) == INVALID
        assert call(bufs.struct(('grad_stats', hist), d_edges, E=0)) == INVALID
    assert call(bufs.struct(('grad_stats',), None, E=3)) == INVALID          # edges announced, none given
    with pytest.raises(_lib.DenseRegError) as e:
        h.call('dr_step_report', C.c_float(LR), C.c_float(DIV), C.c_float(CLIP), C.c_int64(0), C.byref(good), be.stream)
    assert e.value.code == INVALID and 'step' in str(e.value)
    # an inference handle
    hi = be.handle(_cfg(), 1)
    assert call(good, handle=hi._h) == STATE
    hi.close()
    be.sync()
    bufs.read(())                                                            # no rejected call wrote anything
    # after all that the handle still works
    got = step_report(be, h, want=('global_counts',))
    assert got['global_counts'][0] == 5


# ---------------------------------------------------------------------------------------------
# 7. Python layer
# ---------------------------------------------------------------------------------------------
def test_hist_edges_and_edge_checks_on_the_host():
    """hist_edges(): symmetric, strictly ascending, finite, float32, 2 ceil(log(hi/lo) / log(ratio)) edges, within the cap of 2048 by
    default; edges that are not strictly ascending or not finite are refused before anything reaches the device."""
    from densereg_amd.engine import Engine, hist_edges
    e = hist_edges()
    assert e.dtype == np.float32 and e.size == 2 * math.ceil(math.log(1e20 / 1e-12) / math.log(1.1)) <= _lib.STEP_REPORT_MAX_EDGES
    assert np.all(np.diff(e) > 0) and np.all(np.isfinite(e)) and np.array_equal(e, -e[::-1])
    assert e[e.size // 2] == np.float32(1e-12) and e[-1] == np.float32(1e20)
    assert np.all(np.abs(e[e.size // 2 + 1:] / e[e.size // 2:-1] / 1.1 - 1.0) < 1e-3)      # the ratio, up to the rounding of the count
    small = hist_edges(1e-3, 1.0, 2.0)
    assert small.size == 20 and small[-1] == 1.0
    with pytest.raises(ValueError):
        hist_edges(1e-30, 1e30, 1.01)                                        # more than 2048 edges
    with pytest.raises(ValueError):
        hist_edges(1.0, 0.5)
    fake = types.SimpleNamespace()
    for bad in ([0.0, 1.0, 1.0], [0.0, -1.0], [0.0, float('nan')], [0.0, float('inf')], [], np.arange(2049.0)):
        with pytest.raises(ValueError):
            Engine._device_edges(fake, bad)
    assert Engine._device_edges(fake, None) is None
    assert set(_lib.STEP_REPORT_FIELDS) == {n[:-4] for n, _ in _lib.DrStepReport._fields_[2:]}


@pytest.mark.gpu
def test_engine_and_trainer_step_report_interface(gpu):
    """Engine.step_report: field selection, shapes, dtypes, names in dr_param_info's order, edges; DataParallelTrainer.step_report
    describes the step its next optimizer_step takes."""
    import torch
    from densereg_amd.engine import Engine, StepReport, hist_edges
    from densereg_amd.model import hourglass_um_crop_tiny as M
    from densereg_amd.parallel import DataParallelTrainer, learning_rate
    from densereg_amd.data.synthetic import make_crops
    B = 2
    eng = Engine(NET[0], NET[1], NET[2], NET[3], 3, B, 0, True)
    names = tuple(n for n, _, tr in eng.param_infos() if tr)
    V = len(names)
    assert names == tuple(_layout()[0])
    eng.load_params(M._random_params(eng))
    eng.zero_grad()
    rep = eng.step_report(1e-3, 2.0, 1)
    assert isinstance(rep, StepReport) and rep.names == names and rep.edges is None
    assert rep.grad_hist is None and rep.param_hist is None
    for n in FIELDS:
        if n in HISTS:
            continue
        a = rep.get(n)
        assert tuple(a.shape) == _shape(n, 0) and a.dtype == (torch.int32 if _lib.STEP_REPORT_FIELDS[n][1] else torch.float32), n
    assert rep.global_counts.tolist() == [0, 0, int(_layout()[1].sum())]     # a zeroed accumulator: everything zero, nothing clipped
    edges = hist_edges()
    rep2 = eng.step_report(1e-3, 2.0, 1, fields=('grad_hist', 'global'), edges=edges)
    assert tuple(rep2.grad_hist.shape) == (V, edges.size + 1) and rep2.param_stats is None and rep2.param_hist is None
    assert torch.equal(rep2.global_, rep.global_) and torch.equal(rep2.edges.cpu(), torch.from_numpy(edges))
    assert rep2.grad_hist[:, edges.size // 2].tolist() == _layout()[1].tolist()      # g = 0: the bucket between -lo and +lo
    rep3 = eng.step_report(1e-3, 2.0, 1, fields=('param_hist',), edges=rep2.edges)   # the device edges of an earlier report
    assert int(rep3.param_hist.sum()) == int(_layout()[1].sum())
    with pytest.raises(ValueError):
        eng.step_report(1e-3, 2.0, 1, fields=('no_such_member',))
    with pytest.raises(ValueError):
        eng.step_report(1e-3, 2.0, 1, fields=('grad_hist',))
    with pytest.raises(ValueError):
        eng.step_report(1e-3, 2.0, 1, edges=[0.0, 0.0])
    # the trainer: the report after the window's micro-steps is the step optimizer_step then takes
    trainer = DataParallelTrainer(eng, dataset='icvl', sub_batch=2)
    trainer.report_every(1, ('update_stats', 'global', 'global_counts'))
    dm, poses, cfgs, coms, _ = make_crops(B, 'icvl', seed=5, hw=NET[3])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu.device)
    ndm = eng.norm_dm(t(dm), t(coms))
    args = (ndm, t(np.ascontiguousarray(poses[:, :3 * NET[2]])), t(cfgs), t(coms))
    theta0 = eng.flat_view('param').clone()
    trainer.micro_step(*args, seed=0)
    assert trainer.take_step_report() is None
    mid = trainer.step_report(('global',))                                   # one rank: any time
    assert float(mid.global_[0]) > 0
    trainer.micro_step(*args, seed=1)
    step, last = trainer.take_step_report()
    assert step == 1 and trainer.global_step == 1 and trainer.take_step_report() is None
    du = (theta0.double() - eng.flat_view('param').double()).norm()
    assert abs(float(last.global_[3]) / float(du) - 1.0) < 1e-5 and int(last.global_counts[0]) == 0
    assert learning_rate(0, 'icvl', B, 2) == 1e-3
    torch.cuda.synchronize()
    del trainer
    eng.close()


# ---------------------------------------------------------------------------------------------
# 8. the driver
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('every', [1, 0])
def test_driver_step_report_flag(gpu, every, tmp_path, monkeypatch):
    """--step_report 1 --max_steps 3 on the synthetic NYU set: three report lines and a normal end; with the flag at 0 none."""
    from densereg_amd import flags
    from densereg_amd.model import hourglass_um_crop_tiny as M
    from densereg_amd.network import um_v1
    monkeypatch.chdir(tmp_path)
    flags.parse(['--dataset', 'nyu', '--num_stack', '1', '--fea_num', '16', '--is_train', 'True', '--batch_size', '2', '--sub_batch', '2',
                 '--max_steps', '3', '--synthetic_crops', '8', '--step_report', str(every)])
    try:
        eng = um_v1.get_engine(14, 128, 2, 0, True)
        eng.load_params(M._random_params(eng))
        model = M.JointDetectionModel(M.SyntheticDataset('nyu', 'training'), um_v1.detect_net, epoch=1, net_desc=um_v1.TOWER_NAME)
        log = io.StringIO()
        trainer = M.train(model, None, log=log)
        lines = [ln for ln in log.getvalue().splitlines() if 'step report' in ln]
        assert trainer.global_step == 3
        assert len(lines) == (3 if every else 0), log.getvalue()
        for k, ln in enumerate(lines):
            assert 'step report %d:' % (k + 1) in ln and 'clipped' in ln and 'zero' in ln and 'nan' not in ln.lower(), ln
    finally:
        flags.parse([])
