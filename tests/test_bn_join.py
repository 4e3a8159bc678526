"""Projection residuals (um_v1.py:18-48 with num_out != cin) with their two BatchReNorm branches joined in one pass: the skip conv
runs conv + statistics + finalize and no apply pass, the module's last conv forms ``relu(bn(raw_3)) + relu(bn(raw_s))`` in its
forward apply and the skip conv's backward sums in its backward apply (train_kernels.h: bn_train_join_kernel, bn_bwd_join_kernel;
train_exec.inc: plan_backward).  ``DR_BN_JOIN=0`` keeps the two-pass form.

* kernel level, through ``dr_dbg_bn_join``, which fills the parameters and calls the launchers the executors call (train_kernels.h:
  bn_form, launch_bn_fwd_apply / _join, launch_bn_bwd_reduce / _apply / _join -- form, grids and kernel instances are theirs): both
  forms against an fp64 autograd of the pair (1e-5 of each tensor's max, the bound of tests/test_bn_layer.py), and the joined output
  bit-equal to the two-pass one;
* network level: one training step, joined against two-pass (losses and module outputs bit-equal) and against the oracle's fp64
  autograd taking the engine's switches (the bar of tests/test_train_parity.py's switch-free gradient test);
* ``dr_read_activation`` of a joined skip conv, which the forward no longer stores;
* the plan: how many pairs are joined, from the ``DR_DEBUG_PLAN`` line.

``[emu]`` on CPU fibers, ``[gpu]`` on an MI355X.
"""
import ctypes as C
import re

import numpy as np
import pytest

from densereg_amd import _lib
from tests.common import flat_grads_by_name, grad_metrics

BACKENDS = [pytest.param('emu'), pytest.param('gpu', marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def be(request):
    return request.getfixturevalue(request.param)


# ---- 1. the pair of layers ---------------------------------------------------------------------------------------------------------

def _pair_reference(xs, ws, x3, w3, par, r_max, d_max, dout, G):
    """fp64 autograd of dst = relu(bn(x_3 w_3)) + relu(bn(x_s w_s)), train-mode BatchReNorm per micro-batch group
    (network/slim/ops.py:130-171: biased moments, eps inside the sqrt, r / d clipped and stop-gradient).  Group g > 0 clips against
    the moving statistics group g-1 left: with zero-debias the first update of the chain leaves the batch moments themselves."""
    import torch
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    M = xs.shape[0]
    Mg = M // G
    raws, outs, leaves = {}, {}, {}
    for l, (x, w) in (('s', (xs, ws)), ('3', (x3, w3))):
        raw = (t(x) @ t(w)).detach().requires_grad_(True)
        gam, bet = t(par['gamma_' + l]).requires_grad_(True), t(par['beta_' + l]).requires_grad_(True)
        mm, mv = t(par['mm_' + l]), t(par['mv_' + l])
        ys = []
        for g in range(G):
            r_ = raw[g * Mg:(g + 1) * Mg]
            mean = r_.mean(0)
            var = ((r_ - mean) ** 2).mean(0)
            std = torch.sqrt(var + 1e-3)
            mstd = torch.sqrt(mv + 1e-3)
            r = torch.clamp(std / mstd, 1.0 / r_max, r_max).detach()
            d = torch.clamp((mean - mm) / mstd, -d_max, d_max).detach()
            ys.append(torch.relu(((r_ - mean) / std * r + d) * gam + bet))
            mm, mv = mean.detach(), var.detach()
        raws[l], outs[l], leaves[l] = raw, torch.cat(ys, 0), (gam, bet)
    dst = outs['3'] + outs['s']
    (dst * t(dout)).sum().backward()
    n = lambda v: v.detach().numpy()
    ref = dict(dst=n(dst))
    for l in ('s', '3'):
        ref['raw_' + l], ref['draw_' + l] = n(raws[l]), n(raws[l].grad)
        ref['dgamma_' + l], ref['dbeta_' + l] = n(leaves[l][0].grad), n(leaves[l][1].grad)
    return ref


def _run_pair(be, Cout, G, joined, seed, B=2, H=5, W=7, Cin_s=19, Cin_3=10, r_max=3.0, d_max=5.0):
    rng = np.random.default_rng(seed)
    M, cs = B * H * W, -(-Cout // 4) * 4
    inp = {}
    for l, Cin in (('s', Cin_s), ('3', Cin_3)):
        inp['x_' + l] = rng.standard_normal((M, Cin)).astype(np.float32)
        inp['w_' + l] = (rng.standard_normal((Cin, Cout)) / np.sqrt(Cin)).astype(np.float32)
        inp['gamma_' + l] = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
        inp['beta_' + l] = (0.3 * rng.standard_normal(Cout)).astype(np.float32)
        inp['mm_' + l] = (0.4 * rng.standard_normal(Cout)).astype(np.float32)          # some channels clip r / d, others do not
        inp['mv_' + l] = rng.uniform(0.05, 4.0, Cout).astype(np.float32)
    dout = rng.standard_normal((M, Cout)).astype(np.float32)

    def padded(a, stride, fill=np.nan):                      # pad channels are poison: must not be read
        out = np.full(a.shape[:-1] + (stride,), fill, np.float32)
        out[..., :a.shape[-1]] = a
        return out
    xs_cs, x3_cs = -(-Cin_s // 4) * 4, -(-Cin_3 // 4) * 4
    d = {n: be.dev(v) for n, v in inp.items() if not n.startswith('x_')}
    d['x_s'], d['x_3'] = be.dev(padded(inp['x_s'], xs_cs)), be.dev(padded(inp['x_3'], x3_cs))
    d_dout = be.dev(padded(dout, cs))
    o = {n: be.dev(np.full((M, cs), -777.0, np.float32)) for n in ('dst', 'raw_s', 'raw_3', 'draw_s', 'draw_3')}
    ov = {n: be.dev(np.zeros(Cout, np.float32)) for n in ('dgamma_s', 'dbeta_s', 'dgamma_3', 'dbeta_3')}
    p = lambda n: be.ptr(d[n])
    a = _lib.DbgBnJoinArgs(B, H, W, Cin_s, Cin_3, Cout, G, int(joined), p('x_s'), xs_cs, p('w_s'), p('x_3'), x3_cs, p('w_3'),
                           p('gamma_s'), p('beta_s'), p('mm_s'), p('mv_s'), p('gamma_3'), p('beta_3'), p('mm_3'), p('mv_3'),
                           r_max, d_max, be.ptr(d_dout), be.ptr(o['dst']), be.ptr(o['raw_s']), be.ptr(o['raw_3']),
                           be.ptr(o['draw_s']), be.ptr(o['draw_3']), be.ptr(ov['dgamma_s']), be.ptr(ov['dbeta_s']),
                           be.ptr(ov['dgamma_3']), be.ptr(ov['dbeta_3']), 0)
    rc = be.dbg.dr_dbg_bn_join(C.byref(a), be.stream)
    assert rc == 0, rc
    be.sync()
    full_dst = be.host(o['dst']).reshape(M, cs)
    assert np.all(full_dst[:, Cout:] == -777.0), 'the apply pass wrote outside its channel range'
    got = {n: be.host(v).reshape(M, cs)[:, :Cout].copy() for n, v in o.items()}
    got.update({n: be.host(v).copy() for n, v in ov.items()})
    assert (a.part_rows > 0) == bool(joined)
    return inp, dout, got, a.part_rows


@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('Cout', [18, 64, 256])
def test_pair_joined_and_two_pass_against_fp64(be, Cout, groups):
    """(B, H, W) = (2, 5, 7): 70 rows, so every workgroup pass has tail rows and the apply grid has several workgroups; Cout = 18: a
    ragged last channel group (and 51 rows per workgroup pass, one idle thread), 64: 16 channel groups per row, 256: 64 per row; one
    batch and two micro-batch groups of 35 rows.  dst, draw_3, draw_s, dbeta and dgamma of both layers of BOTH forms within 1e-5 of
    each tensor's max of the fp64 definition; the joined dst bit-equal to the two-pass dst."""
    seed = 4000 + 10 * Cout + groups
    inp, dout, got_j, rows = _run_pair(be, Cout, groups, True, seed)
    _, _, got_t, _ = _run_pair(be, Cout, groups, False, seed)
    par = {k: v for k, v in inp.items() if k[0] in 'gbm'}
    ref = _pair_reference(inp['x_s'], inp['w_s'], inp['x_3'], inp['w_3'], par, 3.0, 5.0, dout, groups)
    for form, got in (('joined', got_j), ('two-pass', got_t)):
        for name in ('raw_s', 'raw_3', 'dst', 'draw_3', 'draw_s', 'dbeta_3', 'dgamma_3', 'dbeta_s', 'dgamma_s'):
            sc = np.abs(ref[name]).max() + 1e-12
            err = np.abs(got[name] - ref[name]).max() / sc
            print('%s %s: %.3e of the tensor max (Cout %d, groups %d, %d joined rows)' % (form, name, err, Cout, groups, rows))
            assert err <= 1e-5, (form, name, err)
    np.testing.assert_array_equal(got_j['dst'], got_t['dst'])


# ---- 2. / 3. the network ------------------------------------------------------------------------------------------------------------

def _projection_pairs(cfg):
    """(skip conv, last conv) scope names of every projection residual, from the graph walk: c1 (1x1, cin -> cin/2), c2, c3 (1x1 ->
    num_out), then the skip conv (1x1, cin -> num_out) when num_out != cin (oracle/graph.py: walk_residual)."""
    from oracle.graph import conv_specs
    specs = conv_specs(cfg)
    pairs = []
    for i in range(2, len(specs) - 1):
        c1, c3, cs = specs[i - 2], specs[i], specs[i + 1]
        if (c1.k == 1 and c3.k == 1 and cs.k == 1 and c1.bn and c3.bn and cs.bn and c1.cout == c1.cin // 2 and c3.cin == c1.cout and
                cs.cin == c1.cin and cs.cout == c3.cout and c3.cout != c1.cin and specs[i - 1].cin == specs[i - 1].cout == c1.cout):
            pairs.append((cs.name, c3.name))
    return pairs


def _train_step(be, cfg, params, data, G, join, monkeypatch):
    """forward + loss + backward on a fresh handle; returns (handle, losses [G][4], {module output}, gradients by name)."""
    monkeypatch.setenv('DR_BN_JOIN', '1' if join else '0')               # read when the handle plans its backward sweep
    ndm, poses, cfgs, coms = data
    B = ndm.shape[0]
    h = be.handle(cfg, B, training=True)
    h.load_params(params)
    h.call('dr_finalize_params', be.stream)
    h.call('dr_zero_grad', be.stream)
    if G > 1:
        h.call('dr_set_groups', G)
    d = [be.dev(np.ascontiguousarray(a)) for a in data]
    d_lo = be.empty((G, 4))
    h.call('dr_forward_train', B, be.ptr(d[0]), 0, None, C.c_uint64(0), be.stream)
    h.call('dr_loss', B, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), be.ptr(d[3]), be.ptr(d_lo), be.stream)
    h.call('dr_backward', B, be.stream)
    be.sync()
    from oracle.graph import conv_specs
    specs = {c.name: c for c in conv_specs(cfg)}
    outs = {}
    for _, c3 in _projection_pairs(cfg):
        c = specs[c3]
        outs[c3] = be.read_activation(h, c3, (B, c.h_out, c.w_out, c.cout))
    return h, be.host(d_lo).reshape(G, 4).copy(), outs, flat_grads_by_name(be, h, cfg)


def _group_switches(be, h, cfg, B, G, g):
    """tests/test_train_parity.py::_engine_switches for the crops of micro-batch group g: a BatchReNorm layer's ReLU from its raw
    output and the multiply-add the forward applied to THAT group's rows."""
    from oracle.graph import conv_specs
    specs = {c.name: c for c in conv_specs(cfg)}
    Bg = B // G
    sl = slice(g * Bg, (g + 1) * Bg)

    # the sign the engine saw: of the exact raw * scale + shift on the GPU (one fused multiply-add; exact in fp64 up to the last
    # rounding, which keeps the sign), of the twice-rounded fp32 expression on the emulator (built without contraction)
    wide = np.float32 if be.name == 'emu' else np.float64

    def relu(name):
        c = specs[name]
        if c.bn:
            raw = be.read_activation(h, name + '#raw', (B, c.h_out, c.w_out, c.cout))[sl].astype(wide)
            fold = be.read_activation(h, name + '#fold', (G * 2 * c.cout,)).astype(wide).reshape(G, 2, c.cout)[g]
            return raw * fold[0] + fold[1] > 0
        return be.read_activation(h, name, (B, c.h_out, c.w_out, c.cout))[sl] > 0

    def act(name):
        c = specs[name]
        return be.read_activation(h, name, (B, c.h_out, c.w_out, c.cout))[sl]
    return {'relu': relu, 'act': act}


# the bar tests/test_train_parity.py::test_gradient_without_switches_single_stack applies: relative L2 per gradient tensor
SWITCH_FREE_BAR = 1e-4


# (two groups on the emulator: 16 crops of this network are four minutes of CPU fibers -- it passed there, 2.2e-5 on the worst tensor,
# and is not part of the CPU suite; the pair test above runs the grouped kernels on the emulator)
@pytest.mark.parametrize('backend, groups', [pytest.param('emu', 1), pytest.param('gpu', 1, marks=pytest.mark.gpu),
                                             pytest.param('gpu', 2, marks=pytest.mark.gpu)])
def test_training_step_joined_against_two_pass_and_the_fp64_oracle(request, backend, groups, monkeypatch):
    """S=1 F=64 at 128x128, one training step (forward, loss, backward), ``DR_BN_JOIN`` on and off.  One batch: B = 2.  Two micro-batch
    groups: B = 16 -- the executors cut every statistics launch at the group boundary in whole 32-row tiles, and the hourglass
    bottom has four pixels per crop, so eight crops per group is the smallest window they accept (B = 2 in two groups is rejected
    by dr_forward_train).  Losses and the output of every projection residual bit-equal between the two forms; the gradient of both
    forms within the switch-free bar of the oracle's fp64 autograd (the oracle's chained micro-steps for two groups, taking the
    engine's ReLU / max-pool decisions), and the two forms within that bar of each other."""
    import torch
    from oracle import net, train
    from tests.test_train_parity import _case
    be = request.getfixturevalue(backend)
    B = 2 if groups == 1 else 16
    cfg, params, ndm, poses, cfgs, coms = _case(1, 64, 4, B)
    data = (ndm, poses, cfgs, coms)
    assert len(_projection_pairs(cfg)) == 4
    h_j, lo_j, out_j, g_j = _train_step(be, cfg, params, data, groups, True, monkeypatch)
    h_t, lo_t, out_t, g_t = _train_step(be, cfg, params, data, groups, False, monkeypatch)
    np.testing.assert_array_equal(lo_j, lo_t)
    for name in out_j:
        np.testing.assert_array_equal(out_j[name], out_t[name], err_msg=name)
    # the oracle: G chained micro-steps (BatchReNorm state update between them), each with the joined engine's switches
    p = {k: v.copy() for k, v in params.items()}
    shadow, g64, Bg = {}, None, B // groups
    for g in range(groups):
        sl = slice(g * Bg, (g + 1) * Bg)
        lo, gr, upd, _ = train.loss_and_grads(cfg, p, ndm[sl], poses[sl], cfgs[sl], coms[sl], dtype=torch.float64,
                                              switches=_group_switches(be, h_j, cfg, B, groups, g))
        np.testing.assert_allclose(lo_j[g], [lo[k] for k in ('hm', 'hm3', 'um', 'reg')], rtol=2e-5)
        g64 = gr if g64 is None else {k: g64[k] + gr[k] for k in gr}
        net.bn_state_update(p, upd, zero_debias=True, shadow=shadow)
    for form, got in (('joined', g_j), ('two-pass', g_t)):
        names, _, l2, cos = grad_metrics(got, g64)
        w = int(np.argmax(l2))
        print('%s gradient vs the fp64 oracle with the engine\'s switches, per tensor rel-L2: max %.2e (%s) median %.2e | cosine min %.9f'
              % (form, l2.max(), names[w], np.median(l2), cos.min()))
        assert l2.max() < SWITCH_FREE_BAR, (form, l2.max(), names[w])
    names, _, l2, _ = grad_metrics(g_j, g_t)
    print('joined vs two-pass gradient, per tensor rel-L2: max %.2e (%s)' % (l2.max(), names[int(np.argmax(l2))]))
    assert l2.max() < SWITCH_FREE_BAR, (l2.max(), names[int(np.argmax(l2))])
    h_j.close()
    h_t.close()


@pytest.mark.parametrize('backend, groups', [pytest.param('emu', 1), pytest.param('gpu', 1, marks=pytest.mark.gpu),
                                             pytest.param('gpu', 2, marks=pytest.mark.gpu)])
def test_read_activation_of_a_joined_skip_conv(request, backend, groups, monkeypatch):
    """The training forward does not store a joined skip conv's activation; dr_read_activation rebuilds it on request: bit-equal to
    max(raw * scale + shift, 0) from "#raw" and "#fold" -- one rounding on the GPU (the kernels' fused multiply-add: the product of
    two fp32 values is exact in fp64), two on the emulator (built without contraction) -- and to what the two-pass form stored.
    Two micro-batch groups (B = 16, the smallest window the executors accept: see the training-step test above): the rebuilding
    launch takes the executors' grouped grid, "#fold" is [G][2][C] and the rows of group g take the coefficients of group g."""
    from oracle.graph import conv_specs
    from tests.test_train_parity import _case
    be = request.getfixturevalue(backend)
    B = 16 if groups == 2 else 1 if be.name == 'emu' else 2
    Bg = B // groups
    cfg, params, ndm, poses, cfgs, coms = _case(1, 64, 4, B)
    specs = {c.name: c for c in conv_specs(cfg)}
    got = {}
    for join in (True, False):
        monkeypatch.setenv('DR_BN_JOIN', '1' if join else '0')
        h = be.handle(cfg, B, training=True)
        h.load_params(params)
        h.call('dr_finalize_params', be.stream)
        if groups > 1:
            h.call('dr_set_groups', groups)
        d_dm = be.dev(ndm)
        h.call('dr_forward_train', B, be.ptr(d_dm), 0, None, C.c_uint64(0), be.stream)
        be.sync()
        for cs, _ in _projection_pairs(cfg):
            c = specs[cs]
            shape = (B, c.h_out, c.w_out, c.cout)
            y = be.read_activation(h, cs, shape)
            got[(cs, join)] = y
            if join:
                raw = be.read_activation(h, cs + '#raw', shape)
                fold = be.read_activation(h, cs + '#fold', (groups * 2 * c.cout,)).reshape(groups, 2, c.cout)
                for g in range(groups):
                    sl = slice(g * Bg, (g + 1) * Bg)
                    if be.name == 'emu':
                        want = np.maximum(raw[sl] * fold[g, 0] + fold[g, 1], np.float32(0))
                    else:
                        want = np.maximum((raw[sl].astype(np.float64) * fold[g, 0].astype(np.float64) + fold[g, 1].astype(np.float64))
                                          .astype(np.float32), np.float32(0))
                    assert want.dtype == np.float32 and (want > 0).any()
                    np.testing.assert_array_equal(y[sl], want, err_msg='%s, group %d' % (cs, g))
                if groups > 1:
                    assert not np.array_equal(fold[0], fold[1]), cs       # (the groups' coefficients do differ: the slices above matter)
        h.close()
    for cs, _ in _projection_pairs(cfg):
        np.testing.assert_array_equal(got[(cs, True)], got[(cs, False)], err_msg=cs)


# ---- 4. the plan --------------------------------------------------------------------------------------------------------------------

def _joined_pairs(emu, capfd, monkeypatch, S, F, J, join_env=None, bf16=False):
    from oracle.graph import NetConfig
    monkeypatch.setenv('DR_DEBUG_PLAN', '1')
    if join_env is None:
        monkeypatch.delenv('DR_BN_JOIN', raising=False)
    else:
        monkeypatch.setenv('DR_BN_JOIN', join_env)
    capfd.readouterr()
    h = emu.handle(NetConfig(S, F, J), 1, training=True)
    if bf16:
        h.call('dr_set_precision', 1)
    h.close()
    lines = [ln for ln in capfd.readouterr().err.splitlines() if 'plan_backward' in ln]
    assert lines, 'no DR_DEBUG_PLAN line'
    m = re.search(r'projection residuals joined: (\d+)', lines[-1])
    assert m, lines[-1]
    return int(m.group(1))


def test_plan_joins_every_projection_residual(emu, capfd, monkeypatch):
    """CPU: the DR_DEBUG_PLAN line.  S=2 F=128 J=14 (the headline network): conv_2, hg_ins and, per stack, hm3, um_a, um_m = 8 pairs;
    S=1 F=64 J=16: hg_ins is an identity-skip module there, 4 pairs; none with DR_BN_JOIN=0; none on the bf16 path."""
    assert _joined_pairs(emu, capfd, monkeypatch, 2, 128, 14) == 8
    assert _joined_pairs(emu, capfd, monkeypatch, 1, 64, 16) == 4
    assert _joined_pairs(emu, capfd, monkeypatch, 2, 128, 14, join_env='0') == 0
    assert _joined_pairs(emu, capfd, monkeypatch, 1, 64, 16, join_env='0') == 0
    assert _joined_pairs(emu, capfd, monkeypatch, 2, 128, 14, bf16=True) == 0
