"""ctypes binding of ``libdensereg_hip.so`` (the C ABI of ``include/densereg.h``).

The product path has no CPU fallback: if the HIP library is missing this module raises at load
time with build instructions, and ``dr_create`` itself fails when no gfx950 device is present.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DR_LIB_VARIANT=<name> (measurement only): load lib/variants/<name>/ instead -- the same sources built with other -D switches
# (tools/build_variants.sh), so that compile-time experiments can be A/B-ed in one GPU visit.  Unset = the product.
_LIBDIR = os.path.join(_HERE, 'lib', 'variants', os.environ['DR_LIB_VARIANT']) if os.environ.get('DR_LIB_VARIANT') else os.path.join(_HERE, 'lib')
LIB_PATH = os.path.join(_LIBDIR, 'libdensereg_hip.so')
DEBUG_LIB_PATH = os.path.join(_LIBDIR, 'libdensereg_hip_dbg.so')      # product sources + dr_dbg_* hooks (tests/, tools/)

DR_OK = 0
DROPOUT_OFF, DROPOUT_MASK, DROPOUT_RNG = 0, 1, 2


class DrConfig(C.Structure):
    _fields_ = [('num_stack', C.c_int32), ('num_fea', C.c_int32), ('num_jnt', C.c_int32), ('in_hw', C.c_int32),
                ('kernel_size', C.c_int32), ('max_batch', C.c_int32), ('device', C.c_int32), ('training', C.c_int32)]


class DrVoteReport(C.Structure):
    """include/densereg.h: struct dr_vote_report -- device addresses, None / 0 = member not wanted."""
    _fields_ = [(n, C.c_void_p) for n in ('xyz_norm_dev', 'uvd_dev', 'can_idx_dev', 'can_score_dev', 'can_pts_dev',
                                           'ori_pts_dev', 'can_weight_dev', 'mass_dev', 'hm_peak_dev')]


# member of DrVoteReport without its _dev suffix -> (trailing shape after (B, J), is_int32)
VOTE_REPORT_FIELDS = {'xyz_norm': ((3,), False), 'uvd': ((3,), False), 'can_idx': ((5,), True), 'can_score': ((5,), False),
                      'can_pts': ((5, 3), False), 'ori_pts': ((5, 3), False), 'can_weight': ((5,), False), 'mass': ((), False),
                      'hm_peak': ((3,), False)}


class DrLossReport(C.Structure):
    """include/densereg.h: struct dr_loss_report -- device addresses, None / 0 = member not wanted."""
    _fields_ = [(n, C.c_void_p) for n in ('total_dev', 'stack_losses_dev', 'joint_losses_dev', 'crop_losses_dev', 'gt_hm_dev',
                                           'gt_hm3_dev', 'gt_um_dev')]


# member of DrLossReport without its _dev suffix -> shape rule f(B, S, J, m), m = map side
LOSS_REPORT_FIELDS = {'total': lambda B, S, J, m: (3,), 'stack_losses': lambda B, S, J, m: (S, 3),
                      'joint_losses': lambda B, S, J, m: (S, J, 3), 'crop_losses': lambda B, S, J, m: (B, S, 3),
                      'gt_hm': lambda B, S, J, m: (B, m, m, J), 'gt_hm3': lambda B, S, J, m: (B, m, m, J),
                      'gt_um': lambda B, S, J, m: (B, m, m, 3 * J)}


class DrStepReport(C.Structure):
    """include/densereg.h: struct dr_step_report -- the edges in, device addresses out, None / 0 = member not wanted."""
    _fields_ = [('hist_edges_dev', C.c_void_p), ('num_edges', C.c_int32)] + [(n, C.c_void_p) for n in (
        'param_stats_dev', 'grad_stats_dev', 'raw_stats_dev', 'update_stats_dev', 'grad_counts_dev', 'global_dev',
        'global_counts_dev', 'grad_hist_dev', 'param_hist_dev')]


# output member of DrStepReport without its _dev suffix -> (shape rule f(V, E), is_int32); V = trainable variables, E = edges
STEP_REPORT_FIELDS = {'param_stats': (lambda V, E: (V, 4), False), 'grad_stats': (lambda V, E: (V, 4), False),
                      'raw_stats': (lambda V, E: (V, 2), False), 'update_stats': (lambda V, E: (V, 4), False),
                      'grad_counts': (lambda V, E: (V, 4), True), 'global': (lambda V, E: (6,), False),
                      'global_counts': (lambda V, E: (3,), True), 'grad_hist': (lambda V, E: (V, E + 1), True),
                      'param_hist': (lambda V, E: (V, E + 1), True)}
STEP_REPORT_MAX_EDGES = 2048


class DrPanel(C.Structure):
    """include/densereg.h: struct dr_panel -- one panel of dr_render_panels."""
    _fields_ = [('src_dev', C.c_void_p)] + [(n, C.c_int32) for n in ('src_h', 'src_w', 'src_c', 'channel', 'kind')] + [
        ('pts_dev', C.c_void_p)] + [(n, C.c_int32) for n in ('num_pts', 'pts_space', 'pts_hw', 'skeleton')] + [('cfg_dev', C.c_void_p)]


PANEL_JET, PANEL_GREYS, PANEL_UM_XY = 0, 1, 2
PTS_NONE, PTS_UVD, PTS_XYZ_MM = 0, 1, 2
SKEL_NONE, SKEL_ICVL, SKEL_NYU, SKEL_MSRA = 0, 1, 2, 3
RENDER_MAX_PANELS = 16


class KernelStat(C.Structure):
    _fields_ = [('name', C.c_char * 64), ('launches', C.c_int64), ('total_ms', C.c_double), ('flops', C.c_double),
                ('bytes', C.c_double)]


class DbgBnArgs(C.Structure):
    """include/densereg_debug.h: dr_dbg_bn_args (test hook)."""
    _fields_ = [('B', C.c_int), ('H', C.c_int), ('W', C.c_int), ('Cin', C.c_int), ('Cout', C.c_int), ('k', C.c_int),
                ('x', C.c_void_p), ('x_cs', C.c_int), ('w', C.c_void_p),
                ('gamma', C.c_void_p), ('beta', C.c_void_p), ('mm', C.c_void_p), ('mv', C.c_void_p),
                ('r_max', C.c_float), ('d_max', C.c_float), ('relu', C.c_int),
                ('res', C.c_void_p), ('dout', C.c_void_p),
                ('gr', C.c_void_p), ('gr_cs', C.c_int), ('wr', C.c_void_p), ('kr', C.c_int), ('Cr', C.c_int),
                ('y', C.c_void_p), ('raw', C.c_void_p), ('bnc', C.c_void_p), ('mm_next', C.c_void_p), ('mv_next', C.c_void_p),
                ('dout_used', C.c_void_p), ('draw', C.c_void_p), ('dgamma', C.c_void_p), ('dbeta', C.c_void_p),
                ('dres', C.c_void_p), ('fwd_rows', C.c_int), ('bwd_rows', C.c_int)]


class DbgBnJoinArgs(C.Structure):
    """include/densereg_debug.h: dr_dbg_bn_join_args (test hook)."""
    _fields_ = [(n, C.c_int) for n in ('B', 'H', 'W', 'Cin_s', 'Cin_3', 'Cout', 'groups', 'joined')] + [
        ('x_s', C.c_void_p), ('xs_cs', C.c_int), ('w_s', C.c_void_p), ('x_3', C.c_void_p), ('x3_cs', C.c_int), ('w_3', C.c_void_p)] + [
        (n, C.c_void_p) for n in ('gamma_s', 'beta_s', 'mm_s', 'mv_s', 'gamma_3', 'beta_3', 'mm_3', 'mv_3')] + [
        ('r_max', C.c_float), ('d_max', C.c_float)] + [
        (n, C.c_void_p) for n in ('dout', 'dst', 'raw_s', 'raw_3', 'draw_s', 'draw_3', 'dgamma_s', 'dbeta_s', 'dgamma_3', 'dbeta_3')] + [
        ('part_rows', C.c_int)]


class DenseRegError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('densereg error %d: %s' % (code, msg))
        self.code = code


_vp, _fp, _i, _sz = C.c_void_p, C.c_void_p, C.c_int, C.c_size_t

# name -> (restype, argtypes); every symbol include/densereg.h declares
SIGNATURES = {
    'dr_abi_version': (_i, []),
    'dr_backend': (C.c_char_p, []),
    'dr_create': (_i, [C.POINTER(DrConfig), C.POINTER(_vp)]),
    'dr_destroy': (None, [_vp]),
    'dr_last_error': (C.c_char_p, [_vp]),
    'dr_param_count': (_i, [_vp]),
    'dr_param_info': (_i, [_vp, _i, C.POINTER(C.c_char_p), C.POINTER(C.c_int32 * 4), C.POINTER(C.c_int32),
                           C.POINTER(C.c_int32)]),
    'dr_load_param': (_i, [_vp, C.c_char_p, _fp, _sz]),
    'dr_read_param': (_i, [_vp, C.c_char_p, _fp, _sz]),
    'dr_finalize_params': (_i, [_vp, _vp]),
    'dr_norm_dm': (_i, [_vp, _i, _fp, _fp, _fp, _vp]),
    'dr_forward_eval': (_i, [_vp, _i, _fp, _fp, _fp, _fp, _vp]),
    'dr_read_maps': (_i, [_vp, _i, _i, _fp, _fp, _fp, _vp]),
    'dr_vote': (_i, [_vp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp]),
    'dr_infer': (_i, [_vp, _i, _fp, _fp, _fp, _fp, _vp]),
    'dr_vote_report': (_i, [_vp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, C.POINTER(DrVoteReport), _vp]),
    'dr_infer_report': (_i, [_vp, _i, _fp, _fp, _fp, _fp, C.POINTER(DrVoteReport), _vp]),
    'dr_targets': (_i, [_vp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp]),
    'dr_loss_report': (_i, [_vp, _i, _fp, _fp, _fp, _fp, C.POINTER(DrLossReport), _vp]),
    'dr_forward_train': (_i, [_vp, _i, _fp, _i, _vp, C.c_uint64, _vp]),
    'dr_loss': (_i, [_vp, _i, _fp, _fp, _fp, _fp, _fp, _vp]),
    'dr_backward': (_i, [_vp, _i, _vp]),
    'dr_zero_grad': (_i, [_vp, _vp]),
    'dr_set_pipeline': (_i, [_vp, _i]),
    'dr_set_groups': (_i, [_vp, _i]),
    'dr_sync_grads': (_i, [_vp, _vp]),
    'dr_flat_grad': (_i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    'dr_flat_param': (_i, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    'dr_apply_adam': (_i, [_vp, C.c_float, C.c_float, C.c_float, C.c_int64, _vp]),
    'dr_step_report': (_i, [_vp, C.c_float, C.c_float, C.c_float, C.c_int64, C.POINTER(DrStepReport), _vp]),
    'dr_read_activation': (_i, [_vp, C.c_char_p, _i, _fp, _sz]),
    'dr_conv_flops_per_crop': (C.c_double, [_vp]),
    'dr_set_precision': (_i, [_vp, _i]),
    'dr_set_fusion': (_i, [_vp, _i]),
    'dr_png_unfilter': (_i, [_vp, _i, _i, _i, _vp]),
    'dr_depth_from_samples': (_i, [_vp, C.c_long, _i, _vp, _vp]),
    'dr_flat_adam': (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    'dr_crc32c': (C.c_uint32, [C.c_uint32, _vp, C.c_size_t]),
    'dr_crop_from_pose': (_i, [_i, _vp, _i, _i, _vp, _i, _vp, _i, C.c_float, _i, _vp, _vp, _vp, _vp]),
    'dr_crop_from_bbx': (_i, [_i, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    'dr_data_aug': (_i, [_i, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dr_render_panels': (_i, [_i, C.POINTER(DrPanel), _i, _i, _vp, _vp]),
    'dr_colormap': (_i, [_i, _vp]),
    'dr_profile_enable': (_i, [_vp, _i]),
    'dr_profile_read': (_i, [_vp, C.POINTER(KernelStat), _i, C.POINTER(_i)]),
    'dr_profile_detail': (_i, [_vp, C.POINTER(KernelStat), _i, C.POINTER(_i)]),
    'dr_lookback_expired': (_i, [_vp]),        # diagnostic of the opt-in BatchReNorm look-back (DR_BN_LOOKBACK=1)
}

# include/densereg_debug.h: test / micro-benchmark hooks.  NOT in the product library: libdensereg_hip_dbg.so (same sources
# + -DDR_DEBUG_HOOKS) and the host emulator export them; tests/ and tools/ load that library for these calls only.
DEBUG_SIGNATURES = {
    'dr_dbg_conv_bench': (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_float)]),
    'dr_dbg_force_tile': (_i, [_i]),
    'dr_dbg_force_bf16': (_i, [_i]),
    'dr_dbg_force_bf16_storage': (_i, [_i]),
    'dr_dbg_force_x3': (_i, [_i]),
    'dr_dbg_p3_launches': (C.c_long, []),
    'dr_dbg_x3h_launches': (C.c_long, []),
    'dr_dbg_bn_finalize_rows': (_i, [_i]),
    'dr_dbg_wgrad_bench': (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_float), C.POINTER(_i)]),
    'dr_dbg_bn_bench': (_i, [C.c_long, _i, _i, _i, C.POINTER(C.c_float)]),
    'dr_dbg_wgrad': (_i, [_i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, C.c_float, _i, _i, _vp, _vp]),
    'dr_dbg_mfma_peak': (_i, [_i, _i, _i, C.POINTER(C.c_float)]),
    'dr_dbg_bn_layer': (_i, [C.POINTER(DbgBnArgs), _vp]),
    'dr_dbg_bn_join': (_i, [C.POINTER(DbgBnJoinArgs), _vp]),
    'dr_dbg_vis_sin': (_i, [_vp, _i, _vp, _vp]),
    'dr_dbg_maxpool':(_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    'dr_dbg_act_dgrad': (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, C.c_float, _vp, _vp, _vp]),
    'dr_dbg_conv2d': (_i, [_i, _i, _i, _i, _i, _i, _fp, _i, _fp, _fp, _fp, _i, _fp, _i, _fp, C.c_float, _fp, _i, _fp, _vp]),
}


def bind(lib: C.CDLL, debug: bool = False) -> C.CDLL:
    sigs = dict(SIGNATURES, **DEBUG_SIGNATURES) if debug else SIGNATURES
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)          # AttributeError if the library misses a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


def load() -> C.CDLL:
    """Load the product library; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                'densereg_amd: %s not found. Build it with `python -c "import __graft_entry__ as g; g.build()"` '
                '(hipcc --offload-arch=gfx950). There is no CPU fallback.' % LIB_PATH)
        _lib = bind(C.CDLL(LIB_PATH))
        if _lib.dr_backend() != b'hip-gfx950':
            raise ImportError('densereg_amd: %s is not the HIP build (backend=%r)' % (LIB_PATH, _lib.dr_backend()))
    return _lib


_dbg = None


def load_debug() -> C.CDLL:
    """The debug build (``libdensereg_hip_dbg.so``: the product's sources + the ``dr_dbg_*`` hooks of
    ``include/densereg_debug.h``).  Only tests/ and tools/ call this; nothing in the package does."""
    global _dbg
    if _dbg is None:
        if not os.path.exists(DEBUG_LIB_PATH):
            raise ImportError('densereg_amd: %s not found (./build.sh builds it next to the product library)' % DEBUG_LIB_PATH)
        _dbg = bind(C.CDLL(DEBUG_LIB_PATH), debug=True)
        if _dbg.dr_backend() != b'hip-gfx950':
            raise ImportError('densereg_amd: %s is not the HIP build' % DEBUG_LIB_PATH)
    return _dbg


class Handle:
    """Thin RAII wrapper over ``dr_handle*``; all pointer arguments are raw addresses (ints)."""

    def __init__(self, lib: C.CDLL, num_stack=2, num_fea=128, num_jnt=16, in_hw=128, kernel_size=3, max_batch=40,
                 device=0, training=False):
        self.lib = lib
        self.cfg = DrConfig(num_stack, num_fea, num_jnt, in_hw, kernel_size, max_batch, device, int(training))
        self._h = _vp()
        rc = lib.dr_create(C.byref(self.cfg), C.byref(self._h))
        if rc != DR_OK:
            raise DenseRegError(rc, (lib.dr_last_error(None) or b'').decode())

    def close(self):
        if self._h:
            self.lib.dr_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != DR_OK:
            raise DenseRegError(rc, (self.lib.dr_last_error(self._h) or b'').decode())

    def call(self, fn_name, *args):
        self.check(getattr(self.lib, fn_name)(self._h, *args))

    # -- variables ---------------------------------------------------------------------------
    def param_infos(self):
        out = []
        for i in range(self.lib.dr_param_count(self._h)):
            name = C.c_char_p()
            dims = (C.c_int32 * 4)()
            nd, tr = C.c_int32(), C.c_int32()
            self.check(self.lib.dr_param_info(self._h, i, C.byref(name), C.byref(dims), C.byref(nd), C.byref(tr)))
            out.append((name.value.decode(), tuple(dims[:nd.value]), bool(tr.value)))
        return out

    def load_params(self, params):
        """params: dict TF-name -> numpy float32 array (host)."""
        import numpy as np
        for name, shape, _ in self.param_infos():
            a = np.ascontiguousarray(params[name], dtype=np.float32)
            assert tuple(a.shape) == tuple(shape), (name, a.shape, shape)
            self.call('dr_load_param', name.encode(), a.ctypes.data, a.size)

    def read_params(self):
        import numpy as np
        out = {}
        for name, shape, _ in self.param_infos():
            a = np.empty(shape, np.float32)
            self.call('dr_read_param', name.encode(), a.ctypes.data, a.size)
            out[name] = a
        return out

    def flat(self, which='param'):
        p, n = _vp(), _sz()
        self.call('dr_flat_' + which, C.byref(p), C.byref(n))
        return p.value, n.value

    def profile(self, on: bool):
        self.call('dr_profile_enable', int(on))

    def profile_read(self):
        arr = (KernelStat * 32)()
        n = _i()
        self.call('dr_profile_read', arr, 32, C.byref(n))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms,
                     flops=arr[i].flops, bytes=arr[i].bytes) for i in range(n.value)]

    def profile_detail(self):
        arr = (KernelStat * 2048)()
        n = _i()
        self.call('dr_profile_detail', arr, 2048, C.byref(n))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms,
                     flops=arr[i].flops, bytes=arr[i].bytes) for i in range(n.value)]

    def conv_flops_per_crop(self):
        return float(self.lib.dr_conv_flops_per_crop(self._h))
