"""ctypes binding of libbhnerf_hip.so (include/bhnerf_hip.h), libbhnerf_kerr.so (include/bhnerf_kerr.h), libbhnerf_eht.so
(include/bhnerf_eht.h), libbhnerf_grf.so (include/bhnerf_grf.h), libbhnerf_eql.so (include/bhnerf_eql.h), libbhnerf_flow.so
(include/bhnerf_flow.h), libbhnerf_rec.so (include/bhnerf_rec.h), libbhnerf_cls.so (include/bhnerf_cls.h), libbhnerf_pol.so
(include/bhnerf_pol.h), libbhnerf_reg.so (include/bhnerf_reg.h) and libbhnerf_jnt.so (include/bhnerf_jnt.h).

PyTorch is used only as the owner of device memory and streams: every call passes raw
``data_ptr()`` addresses and the current HIP stream handle through the C ABI.  There is no CPU
fallback: if the library cannot be loaded, or a call fails, a ``HipError`` is raised.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
# BHNERF_HIP_LIB: an alternative build of the library, e.g. another commit's, to compare against
LIB_PATH = os.environ.get('BHNERF_HIP_LIB') or os.path.join(CSRC, 'libbhnerf_hip.so')

ABI_VERSION = 5              # BHN_ABI_VERSION of include/bhnerf_hip.h this binding was written against
BHN_F32, BHN_BF16, BHN_BF16_T8 = 0, 1, 2
BHN_T8_CALIBRATE = 0x100
BHN_CLK_FWD, BHN_CLK_FWD_TRAIN, BHN_CLK_CHAIN, BHN_CLK_DW, BHN_CLK_SLOTS = 0, 1, 2, 3, 4      # kernel slots of bhn_frames.clock_probe
BHN_TAPE_INFO_N = 8
TAPE_FLAGS = {'drop_h1': 1, 'drop_ga': 2, 'ga0_chain': 4, 'fused128': 8, 'drop_hd': 16, 'lbits': 32, 'general': 64}     # lbits: reserved, never set
MODES = {'f32': BHN_F32, 'fp32': BHN_F32, 'float32': BHN_F32, 'bf16': BHN_BF16, 'bfloat16': BHN_BF16,
         'bf16_t8': BHN_BF16_T8}            # bf16 arithmetic, 8-bit (e4m3) backward tape: include/bhnerf_hip.h


class HipError(RuntimeError):
    pass


class bhn_model(C.Structure):
    _fields_ = [('net_depth', C.c_int32), ('net_width', C.c_int32), ('posenc_deg', C.c_int32),
                ('do_skip', C.c_int32), ('scale', C.c_float), ('rmin', C.c_float), ('rmax', C.c_float),
                ('z_width', C.c_float)]


class bhn_geom(C.Structure):
    _fields_ = [('R', C.c_int64), ('G', C.c_int64), ('S', C.c_int32), ('x', C.c_void_p), ('y', C.c_void_p),
                ('z', C.c_void_p), ('Omega', C.c_void_p), ('t_geo', C.c_void_p), ('w', C.c_void_p),
                ('dom', C.c_void_p), ('groups', C.c_void_p), ('n_groups', C.c_int64), ('ray_idx', C.c_void_p),
                ('n_points', C.c_int64), ('ray_span', C.c_int32)]


class bhn_frames(C.Structure):
    _fields_ = [('B', C.c_int32), ('tM0', C.c_void_p), ('clock_probe', C.c_void_p)]      # clock_probe: NULL unless bench.py measures the kernels' clocks


class bhn_volume_view(C.Structure):
    _fields_ = [('facewidth', C.c_double), ('linewidth', C.c_double), ('bh_radius', C.c_double), ('bh_albedo', C.c_double * 3)]


_P, _I32, _I64, _F, _D, _SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t
_MP, _GP, _FP = C.POINTER(bhn_model), C.POINTER(bhn_geom), C.POINTER(bhn_frames)

# name -> (restype, argtypes); must list every symbol include/bhnerf_hip.h declares
SIGNATURES = {
    'bhn_version': (C.c_int, []),
    'bhn_last_error': (C.c_char_p, []),
    'bhn_param_count': (_I64, [_MP]),
    'bhn_param_layout': (C.c_int, [_MP, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I32)]),
    'bhn_geom_prepare': (C.c_int, [_P, _P, _P, _P, _P, _I32, _I64, _F, _F, _F, _P, _P, _P]),
    'bhn_radiative_transfer_fwd': (C.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _P]),
    'bhn_radiative_transfer_bwd': (C.c_int, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _P]),
    'bhn_packed_bytes': (_SZ, [_MP, _I32]),
    'bhn_pack_weights': (C.c_int, [_MP, _I32, _P, _P, _P]),
    'bhn_predict_fwd': (C.c_int, [_MP, _I32, _P, _GP, _FP, _P, _P]),
    'bhn_render_fwd': (C.c_int, [_MP, _I32, _P, _GP, _FP, _P, _P]),
    'bhn_render_bwd_workspace_bytes': (_SZ, [_MP, _I32, _I32, _I64, _I32]),
    'bhn_render_bwd': (C.c_int, [_MP, _I32, _P, _GP, _FP, _P, _P, _P, _SZ, _P]),
    'bhn_render_fwd_train': (C.c_int, [_MP, _I32, _P, _GP, _FP, _P, _P, _SZ, _P]),
    'bhn_render_bwd_tape': (C.c_int, [_MP, _I32, _P, _GP, _FP, _P, _P, _P, _SZ, _P]),
    'bhn_chi2_image': (C.c_int, [_P, _P, _P, _P, _F, _I32, _I32, _I32, _I64, _P, _P, _P]),
    'bhn_chi2_eht_ws_floats': (_SZ, [_I32, _I32, _I32, _I64]),
    'bhn_chi2_eht': (C.c_int, [_P, _P, _P, _P, _F, _I32, _I32, _I32, _I32, _I64, _P, _P, _P, _P]),
    'bhn_voxel_render_fwd': (C.c_int, [_GP, _FP, _P, _I32, _I32, _I32, _I64, C.POINTER(C.c_float), _P, _P]),
    'bhn_trilinear': (C.c_int, [_P, _I64, _P, _I32, _I32, _I32, C.POINTER(C.c_float), _P, _P]),
    'bhn_grid_predict_fwd': (C.c_int, [_GP, _FP, _P, _I32, _F, _P, _P]),
    'bhn_grid_render_fwd': (C.c_int, [_GP, _FP, _P, _I32, _F, _P, _P]),
    'bhn_grid_render_bwd': (C.c_int, [_GP, _FP, _P, _I32, _F, _P, _P, _P]),
    'bhn_volume_render': (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I64, _P, _I32, C.POINTER(bhn_volume_view), _P, _P]),
    'bhn_adam_step': (C.c_int, [_P, _P, _P, _P, _I64, _I64, _F, _F, _F, _F, _F, _P]),
    'bhn_adam_hyper': (C.c_int, [_I64, _F, _F, _F, C.POINTER(C.c_float)]),
    'bhn_adam_step_dev': (C.c_int, [_P, _P, _P, _P, _I64, _P, _F, _F, _F, _F, _P]),
    'bhn_render_bwd_tape_timed': (C.c_int, [_MP, _I32, _P, _GP, _FP, _P, _P, _P, _SZ, _P, C.POINTER(C.c_void_p), _I32]),
    'bhn_render_bwd_tape_kernel_name': (C.c_char_p, [_I32]),
    'bhn_render_bwd_tape_kernel_name_for': (C.c_char_p, [_MP, _I32, _I32]),
    'bhn_tape_info': (C.c_int, [_MP, _I32, _I64, C.POINTER(_I64), _I32]),
    'bhn_mfma_probe': (C.c_int, [_I32, _I32, _P, _P, _P]),
    'bhn_selftest': (C.c_int, [C.POINTER(_I32), _P, _SZ]),
}

# libbhnerf_kerr.so (include/bhnerf_kerr.h): the Kerr ray tracer, a library of its own beside the hot path's
KERR_LIB_PATH = os.path.join(CSRC, 'libbhnerf_kerr.so')
KERR_SIGNATURES = {
    'bhn_kerr_last_error': (C.c_char_p, []),
    'bhn_kerr_trace': (C.c_int, [_P, _P, _I64, _D, _D, _D, _D, _D, _D, _I32, _I32, _P, _P, _P, _P]),
}

# libbhnerf_eht.so (include/bhnerf_eht.h): the EHT chi-square from (u, v) coordinates, a library of its own as well
EHT_LIB_PATH = os.path.join(CSRC, 'libbhnerf_eht.so')
BHN_EINVAL, BHN_EWORKSPACE = 1, 4
EHT_SIGNATURES = {
    'bhn_eht_last_error': (C.c_char_p, []),
    'bhn_eht_ws_bytes': (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    'bhn_eht_vis': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _D, _D, _P, _P, _SZ, _P]),
    'bhn_eht_chi2_uv': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _D, _D, _I32, _P, _P, _F, _P, _P, _I32, _P, _P, _P, _SZ, _P]),
}

# libbhnerf_grf.so (include/bhnerf_grf.h): Doppler factor and polarised transport factors of kgeo.py, the fourth library
GRF_LIB_PATH = os.path.join(CSRC, 'libbhnerf_grf.so')


class bhn_grf_geos(C.Structure):
    _fields_ = [('n', C.c_int64), ('ngeo', C.c_int32)] + [(k, C.c_void_p) for k in (
        'r', 'theta', 'affine', 'Delta', 'Sigma', 'Xi', 'R', 'Theta', 'lam', 'alpha', 'beta')] + [
        ('spin', C.c_double), ('M', C.c_double), ('E', C.c_double), ('inc', C.c_double)]


_GG = C.POINTER(bhn_grf_geos)
GRF_SIGNATURES = {
    'bhn_grf_last_error': (C.c_char_p, []),
    'bhn_grf_ws_bytes': (_SZ, [_I64, _I32]),
    'bhn_grf_doppler': (C.c_int, [_GG, _P, _D, _I32, _P, _P]),
    'bhn_grf_fluid_field': (C.c_int, [_GG, _P, _D, _D, _D, _P, _P]),
    'bhn_grf_domain_mean': (C.c_int, [_GG, _P, _D, _D, _D, _P, _P, _SZ, _P]),
    'bhn_grf_transport': (C.c_int, [_GG, _P, _P, _P, _P, _D, _D, _D, _P, _P]),
}

# libbhnerf_eql.so (include/bhnerf_eql.h): the equatorial crossings of the image-plane rays, the fifth library
EQL_LIB_PATH = os.path.join(CSRC, 'libbhnerf_eql.so')
EQL_SIGNATURES = {
    'bhn_eql_last_error': (C.c_char_p, []),
    'bhn_eql_crossings': (C.c_int, [_P, _P, _I64, _D, _D, _D, _D, _D, _D, _I32, _I32, _P, _P, _P, _P]),
}

# library name -> (path, signature table, last-error symbol, what bhn_version() must return): the five libraries `make` builds
LIBRARIES = {
    'libbhnerf_hip': (LIB_PATH, SIGNATURES, 'bhn_last_error', ABI_VERSION),
    'libbhnerf_kerr': (KERR_LIB_PATH, KERR_SIGNATURES, 'bhn_kerr_last_error', None),
    'libbhnerf_eht': (EHT_LIB_PATH, EHT_SIGNATURES, 'bhn_eht_last_error', None),
    'libbhnerf_grf': (GRF_LIB_PATH, GRF_SIGNATURES, 'bhn_grf_last_error', None),
    'libbhnerf_eql': (EQL_LIB_PATH, EQL_SIGNATURES, 'bhn_eql_last_error', None),
}

# libbhnerf_flow.so (include/bhnerf_flow.h): (g, J) for a general 4-velocity or the boosted ZAMO, the sixth library.  It is described
# by a tuple of its own, FLOW_LIBRARY, in the layout of the entries of LIBRARIES
FLOW_LIB_PATH = os.path.join(CSRC, 'libbhnerf_flow.so')


class bhn_flow_geos(C.Structure):
    _fields_ = bhn_grf_geos._fields_ + [('omega', C.c_void_p)]


_FG = C.POINTER(bhn_flow_geos)
FLOW_SIGNATURES = {
    'bhn_flow_last_error': (C.c_char_p, []),
    'bhn_flow_zamo_velocity': (C.c_int, [_FG, _D, _D, _P, _P]),
    'bhn_flow_doppler': (C.c_int, [_FG, _P, _D, _I32, _P, _P]),
    'bhn_flow_fluid_field': (C.c_int, [_FG, _P, _D, _D, _D, _P, _P]),
    'bhn_flow_transport': (C.c_int, [_FG, _P, _P, _P, _P, _D, _D, _D, _P, _P]),
    'bhn_flow_transport_zamo': (C.c_int, [_FG, _D, _D, _P, _P, _P, _D, _D, _P, _P]),
}
FLOW_LIBRARY = (FLOW_LIB_PATH, FLOW_SIGNATURES, 'bhn_flow_last_error', None)

# libbhnerf_rec.so (include/bhnerf_rec.h): the geodesic record from the tracer's samples and the Keplerian Omega, the seventh library,
# described like the sixth by a tuple of its own
REC_LIB_PATH = os.path.join(CSRC, 'libbhnerf_rec.so')
REC_FIELDS = ('r', 'theta', 'phi', 't', 'mino', 'Delta', 'Sigma', 'Xi', 'omega', 'x', 'y', 'z', 'R', 'Theta', 'vr', 'vth', 'dtau', 'affine')


class bhn_rec_fields(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in REC_FIELDS]


REC_SIGNATURES = {
    'bhn_rec_last_error': (C.c_char_p, []),
    'bhn_rec_build': (C.c_int, [_P, _P, _P, _I64, _I32, _D, _D, C.POINTER(bhn_rec_fields), _P]),
    'bhn_rec_kepler': (C.c_int, [_P, _I64, _D, _D, _D, _P, _P]),
}
REC_LIBRARY = (REC_LIB_PATH, REC_SIGNATURES, 'bhn_rec_last_error', None)

# libbhnerf_cls.so (include/bhnerf_cls.h): log closure amplitudes and the combined closure loss from (u, v), the eighth library,
# described like the sixth and the seventh by a tuple of its own
CLS_LIB_PATH = os.path.join(CSRC, 'libbhnerf_cls.so')


class bhn_cls_term(C.Structure):
    _fields_ = [('target', C.c_void_p), ('sigma', C.c_void_p), ('weight', C.c_double)]


_CT = C.POINTER(bhn_cls_term)
CLS_SIGNATURES = {
    'bhn_cls_last_error': (C.c_char_p, []),
    'bhn_cls_ws_bytes': (_SZ, [_I32, _I32, _I32, _I32, _I32, _I32]),
    'bhn_cls_chi2': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _D, _D, _CT, _CT, _CT, _P, _P, _I32, _P, _I32, _F, _P, _P, _P, _SZ, _P]),
}
CLS_LIBRARY = (CLS_LIB_PATH, CLS_SIGNATURES, 'bhn_cls_last_error', None)

# libbhnerf_pol.so (include/bhnerf_pol.h): the polarimetric EHT losses 'pvis' and 'm' from (u, v), the ninth library
POL_LIB_PATH = os.path.join(CSRC, 'libbhnerf_pol.so')


class bhn_pol_term(C.Structure):
    _fields_ = [('target', C.c_void_p), ('sigma', C.c_void_p), ('weight', C.c_double)]


_PT = C.POINTER(bhn_pol_term)
POL_SIGNATURES = {
    'bhn_pol_last_error': (C.c_char_p, []),
    'bhn_pol_ws_bytes': (_SZ, [_I32, _I32, _I32, _I32]),
    'bhn_pol_chi2': (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _D, _D, _PT, _PT, _F, _P, _P, _P, _SZ, _P]),
}
POL_LIBRARY = (POL_LIB_PATH, POL_SIGNATURES, 'bhn_pol_last_error', None)

# libbhnerf_reg.so (include/bhnerf_reg.h): the volume priors tv, tsv and l1 on the recovered 3-D emission, the tenth library
REG_LIB_PATH = os.path.join(CSRC, 'libbhnerf_reg.so')
_F3 = C.POINTER(C.c_float)
REG_SIGNATURES = {
    'bhn_reg_last_error': (C.c_char_p, []),
    'bhn_reg_ws_bytes': (_SZ, [_I32, _I32, _I32, _I32]),
    'bhn_reg_loss': (C.c_int, [_P, _I32, _I32, _I32, _I32, _P, _F3, _F3, _F, _F, _P, _P, _P, _P, _SZ, _P]),
}
REG_LIBRARY = (REG_LIB_PATH, REG_SIGNATURES, 'bhn_reg_last_error', None)

# libbhnerf_jnt.so (include/bhnerf_jnt.h): the fan-in of a joint training step (ordered sums of gradients, the terms' losses), the
# eleventh library
JNT_LIB_PATH = os.path.join(CSRC, 'libbhnerf_jnt.so')
BHN_JNT_MAX_TERMS = 8
BHN_JNT_MAX_BLOCKS = 1024    # the cap of the grid of bhn_jnt_sum (include/bhnerf_jnt.h)


class bhn_jnt_ptrs(C.Structure):
    _fields_ = [('p', C.c_void_p * BHN_JNT_MAX_TERMS)]


_JP = C.POINTER(bhn_jnt_ptrs)
JNT_SIGNATURES = {
    'bhn_jnt_last_error': (C.c_char_p, []),
    'bhn_jnt_sum': (C.c_int, [_JP, _I32, _I64, _P, _JP, _P, _P]),
}
JNT_LIBRARY = (JNT_LIB_PATH, JNT_SIGNATURES, 'bhn_jnt_last_error', None)
_loaded = {}                 # path -> handle


def build(verbose=False):
    """Compile the HIP libraries in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(['make', '-C', CSRC, '-j4'], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise HipError('building %s failed (make -C %s)' % (' / '.join(name + '.so' for name in list(LIBRARIES) + ['libbhnerf_flow', 'libbhnerf_rec', 'libbhnerf_cls', 'libbhnerf_pol', 'libbhnerf_reg', 'libbhnerf_jnt']), CSRC))
    return LIB_PATH


def load(path, signatures, abi_version=None):
    """The library at `path` with the restype / argtypes of `signatures` set, loaded once per path; raises HipError (never falls
    back) when it is missing, does not load or lacks a symbol.  abi_version: what its bhn_version() must return."""
    if path not in _loaded:
        if not os.path.exists(path):
            raise HipError('%s not found: run `python -c "import __graft_entry__ as g; g.build()"` '
                           '(or make -C bhnerf_amd/csrc). There is no CPU fallback.' % path)
        try:
            handle = C.CDLL(path)
            if abi_version is not None:      # a stale build would fail later, at a symbol lookup or as "bad mode"
                version = getattr(handle, 'bhn_version', None)
                have = int(version()) if version is not None else -1
                if have != abi_version:
                    raise HipError('%s implements ABI version %d, this package binds version %d: rebuild it (make -C bhnerf_amd/csrc)'
                                   % (path, have, abi_version))
            for name, (res, args) in signatures.items():
                fn = getattr(handle, name)
                fn.restype, fn.argtypes = res, args
        except (OSError, AttributeError) as exc:
            raise HipError('cannot load %s: %s (rebuild it: make -C bhnerf_amd/csrc)' % (path, exc))
        _loaded[path] = handle
    return _loaded[path]


def _lib(library, entry=None):
    """`library` of LIBRARIES, or the library that the tuple `entry` (path, signatures, last-error symbol, ABI version) describes."""
    path, signatures, _, abi_version = entry or LIBRARIES[library]
    return load(path, signatures, abi_version)


def _check(library, rc, entry=None):
    if rc != 0:
        raise HipError('%s: %s (code %d)' % (library, getattr(_lib(library, entry), (entry or LIBRARIES[library])[2])().decode(), rc))


def lib():
    """The loaded library; raises HipError (never falls back) when it is missing or implements another ABI version."""
    return _lib('libbhnerf_hip')


def kerr_lib():
    """The loaded ray-tracer library."""
    return _lib('libbhnerf_kerr')


def eht_lib():
    """The loaded (u, v) EHT library."""
    return _lib('libbhnerf_eht')


def grf_lib():
    """The loaded (g, J) library."""
    return _lib('libbhnerf_grf')


def eql_lib():
    """The loaded equatorial-crossings library."""
    return _lib('libbhnerf_eql')


def flow_lib():
    """The loaded general-flow (g, J) library."""
    return _lib('libbhnerf_flow', FLOW_LIBRARY)


def rec_lib():
    """The loaded geodesic-record library."""
    return _lib('libbhnerf_rec', REC_LIBRARY)


def cls_lib():
    """The loaded closure-loss library."""
    return _lib('libbhnerf_cls', CLS_LIBRARY)


def pol_lib():
    """The loaded polarimetric-loss library."""
    return _lib('libbhnerf_pol', POL_LIBRARY)


def reg_lib():
    """The loaded volume-prior library."""
    return _lib('libbhnerf_reg', REG_LIBRARY)


def jnt_lib():
    """The loaded joint-step fan-in library."""
    return _lib('libbhnerf_jnt', JNT_LIBRARY)


def check(rc):
    _check('libbhnerf_hip', rc)


def kerr_check(rc):
    _check('libbhnerf_kerr', rc)


def eht_check(rc):
    _check('libbhnerf_eht', rc)


def grf_check(rc):
    _check('libbhnerf_grf', rc)


def eql_check(rc):
    _check('libbhnerf_eql', rc)


def flow_check(rc):
    _check('libbhnerf_flow', rc, FLOW_LIBRARY)


def rec_check(rc):
    _check('libbhnerf_rec', rc, REC_LIBRARY)


def cls_check(rc):
    _check('libbhnerf_cls', rc, CLS_LIBRARY)


def pol_check(rc):
    _check('libbhnerf_pol', rc, POL_LIBRARY)


def reg_check(rc):
    _check('libbhnerf_reg', rc, REG_LIBRARY)


def jnt_check(rc):
    _check('libbhnerf_jnt', rc, JNT_LIBRARY)


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipError('device tensor required (the HIP path has no CPU fallback)')


def as_f32(x, device):
    """Contiguous float32 device tensor from array-like input (host->device copy if needed)."""
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32)), device=device)


class _PinnedRing:
    """Small host -> device copies that do not stall the host: a copy from PAGEABLE memory is synchronous on ROCm (the call
    returns only after the stream has reached it, i.e. after every kernel launched before it: one such copy per training step
    -- the frame offsets, the frame indices -- made the host wait for the GPU at every step and then pay the launch latency of
    the next step's ~25 kernels in the open: 0.1-0.5 ms per step).  A ring of pinned staging slots; a slot is re-used only
    after the copy issued from it has executed."""

    def __init__(self, device, slots=32, nbytes=4096):
        self.device, self.nbytes = device, nbytes
        self.slots = [dict(buf=torch.zeros(nbytes, dtype=torch.uint8).pin_memory(), done=None) for _ in range(slots)]
        for sl in self.slots:
            sl['np'] = sl['buf'].numpy()
        self.i = 0

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        n = arr.nbytes
        if n == 0 or n > self.nbytes:
            return torch.as_tensor(arr, device=self.device)
        sl = self.slots[self.i]
        self.i = (self.i + 1) % len(self.slots)
        if sl['done'] is not None:
            sl['done'].synchronize()                 # (waits only when the GPU is a whole ring behind the host)
        else:
            sl['done'] = torch.cuda.Event()
        sl['np'][:n] = arr.reshape(-1).view(np.uint8)
        out = torch.empty(arr.shape, dtype=torch.from_numpy(arr[:0].reshape(-1)).dtype, device=self.device)
        out.view(torch.uint8).reshape(-1).copy_(sl['buf'][:n], non_blocking=True)
        sl['done'].record(torch.cuda.current_stream(self.device))
        return out


_rings = {}


def h2d_small(arr, device):
    """Device tensor with the contents (shape, dtype) of a small NumPy array, through the device's pinned staging ring."""
    device = torch.device(device)
    if device.type != 'cuda':
        return torch.as_tensor(np.ascontiguousarray(arr), device=device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    ring = _rings.get(key)
    if ring is None:
        ring = _rings[key] = _PinnedRing(torch.device('cuda', key[1]))
    return ring.to_device(arr)


def make_model(net_depth, net_width, posenc_deg, do_skip, scale, rmin, rmax, z_width):
    big = 3.0e38
    clip = lambda v: float(min(max(v, -big), big))
    return bhn_model(int(net_depth), int(net_width), int(posenc_deg), int(bool(do_skip)), clip(scale), clip(rmin),
                     clip(rmax), clip(z_width))


def selftest():
    res = (C.c_int32 * 8)()
    scratch = torch.zeros((16384,), dtype=torch.uint8, device='cuda')
    check(lib().bhn_selftest(res, ptr(scratch), scratch.numel()))
    return list(res), lib().bhn_last_error().decode()
