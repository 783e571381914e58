"""GPU tests of the stand-alone kernels (bhnerf_amd/csrc/simple_kernels.hip: geometry fold, radiative transfer, image chi^2,
EHT chi^2, Adam, voxel renderer, trilinear sampler, grid predictor) at the shapes where their branches change, against
float64 references of the float32-rounded inputs.

The cases, their inputs, references, denominators and bounds live in tests/standalone_cases.py; each case's `why` names the
branch it is for, and tests/test_standalone_refs_cpu.py proves on the CPU that each case sees the slips assigned to it at
>= 5x its bound.  Here every case

  * calls the entry point through _hip.lib() directly: the Python wrappers copy their inputs into fresh aligned tensors, and
    the alignment branches (4- and 8-byte aligned sub-views) are under test;
  * writes into outputs embedded in a larger buffer pre-filled with a sentinel and asserts the bytes before and after are
    untouched (all sizes passed are the true sizes);
  * runs twice and asserts bitwise equality where the kernel is documented as reproducible (everything but
    bhn_grid_render_bwd, which adds with float atomics);
  * prints `observed / bound` per output.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gpu_support
import standalone_cases as sc
from gpu_support import dev, lib, place, ptr, stream_ptr as _stream  # noqa: F401

pytestmark = pytest.mark.gpu

BHN_OK, BHN_EINVAL = 0, 1


Out = functools.partial(gpu_support.Out, guard=sc.GUARD, sentinel=sc.SENTINEL)


def twice(run):
    """Run a reproducible kernel twice into fresh outputs: bitwise-equal results, returned once."""
    a, b = run(), run()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    return a


def judge(case, inp, got):
    ref = sc.reference(case, inp)
    errs = sc.errors(case, got, ref, sc.scales(case, inp, ref))
    print(sc.report(case, errs))
    for k, (o, b) in errs.items():
        assert np.isfinite(o) and o <= b, sc.report(case, errs)


def ids(family):
    return [pytest.param(c, id=c.name) for c in sc.BY_FAMILY[family]]


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ids('geom'))
def test_geom_prepare(dev, lib, case):
    inp, p = sc.inputs(case), case.p
    P, S = p['P'], p['S']
    d = {k: place(inp[k], dev) for k in ('coords', 'g', 'dtau', 'Sigma')}
    J = place(inp['J'][:S], dev) if S else None

    def run():
        w, dom = Out(max(S, 1) * P, dev), Out(P, dev, dtype=torch.uint8)
        rc = lib.bhn_geom_prepare(ptr(d['coords']), ptr(d['g']), ptr(d['dtau']), ptr(d['Sigma']), ptr(J), S, P, inp['rmin'], inp['rmax'],
                                  inp['z_width'], ptr(w.view), ptr(dom.view), _stream(dev))
        assert rc == BHN_OK, lib.bhn_last_error()
        torch.cuda.synchronize(dev)
        return dict(w=w.numpy().reshape(max(S, 1), P), dom=dom.numpy())
    judge(case, inp, twice(run))


@pytest.mark.parametrize('case', ids('rt'))
def test_radiative_transfer(dev, lib, case):
    inp, p = sc.inputs(case), case.p
    N, R, G, sh, so = p['N'], p['R'], p['G'], p['shift'], p['shift_out']
    d = {k: place(inp[k], dev, sh) for k in ('e', 'g', 'dtau', 'Sigma', 'dimg')}

    def run():
        img, de = Out(N * R, dev, so), Out(N * R * G, dev, so)
        rc = lib.bhn_radiative_transfer_fwd(ptr(d['e']), ptr(d['g']), ptr(d['dtau']), ptr(d['Sigma']), ptr(img.view), N, R, G, _stream(dev))
        assert rc == BHN_OK, lib.bhn_last_error()
        rc = lib.bhn_radiative_transfer_bwd(ptr(d['dimg']), ptr(d['g']), ptr(d['dtau']), ptr(d['Sigma']), ptr(de.view), N, R, G, _stream(dev))
        assert rc == BHN_OK, lib.bhn_last_error()
        torch.cuda.synchronize(dev)
        return dict(img=img.numpy().reshape(N, R), de=de.numpy().reshape(N, R, G))
    judge(case, inp, twice(run))


@pytest.mark.parametrize('case', ids('chi2'))
def test_chi2_image(dev, lib, case):
    inp, p = sc.inputs(case), case.p
    B, S, R, sh, so = p['B'], p['S'], p['R'], p['shift'], p['shift_out']
    d = {k: place(inp[k], dev, sh) for k in ('images', 'target', 'sigma', 'offset')}
    code = {'full': 0, 'lc': 1}[p['dtype']]

    def run():
        loss = Out(1 + B * S, dev)
        dimg = Out(B * S * R, dev, so) if p['grad'] else None
        rc = lib.bhn_chi2_image(ptr(d['images']), ptr(d['target']), ptr(d['sigma']), ptr(d['offset']), inp['scale'], code, B, S, R,
                                ptr(loss.view), ptr(dimg.view) if dimg else None, _stream(dev))
        assert rc == BHN_OK, lib.bhn_last_error()
        torch.cuda.synchronize(dev)
        l = loss.numpy()
        out = dict(loss0=l[:1].reshape(()), loss_planes=l[1:])
        if dimg:
            out['dimg'] = dimg.numpy().reshape(B, S, R)
        return out
    judge(case, inp, twice(run))


@pytest.mark.parametrize('case', ids('adam'))
def test_adam_step_and_its_device_hyper_twin(dev, lib, case):
    inp, p = sc.inputs(case), case.p
    n, t = p['n'], p['t']
    g = place(inp['g'], dev)
    hp = [inp[k] for k in ('b1', 'b2', 'eps', 'gs')]

    def run(device_hyper):
        st = {k: Out(n, dev, init=inp[k]) for k in ('p', 'm', 'v')}
        if device_hyper:
            h = (C.c_float * 3)()
            assert lib.bhn_adam_hyper(t, inp['lr'], inp['b1'], inp['b2'], h) == BHN_OK
            hyper = place(np.array(list(h), dtype=np.float32), dev)
            rc = lib.bhn_adam_step_dev(ptr(st['p'].view), ptr(g), ptr(st['m'].view), ptr(st['v'].view), n, ptr(hyper), *hp, _stream(dev))
        else:
            rc = lib.bhn_adam_step(ptr(st['p'].view), ptr(g), ptr(st['m'].view), ptr(st['v'].view), n, t, inp['lr'], *hp, _stream(dev))
        assert rc == BHN_OK, lib.bhn_last_error()
        torch.cuda.synchronize(dev)
        return {k: v.numpy() for k, v in st.items()}
    host, device = run(False), run(True)
    for k in host:                                          # bhn_adam_step_dev: bitwise the scalar version's parameters, m, v
        assert np.array_equal(host[k].view(np.uint32), device[k].view(np.uint32)), k
    judge(case, inp, host)


@pytest.mark.parametrize('case', ids('eht'))
def test_chi2_eht(dev, lib, case):
    inp, p = sc.inputs(case), case.p
    N, C_, nvis, R, RS = p['N'], p['C'], p['nvis'], p['R'], p['RS']
    rows = N * C_ * nvis
    assert sc.eht_splits(rows, R) == RS                     # the split this case is for, by the restated rule ...
    ws_n = int(lib.bhn_chi2_eht_ws_floats(N, C_, nvis, R))
    assert ws_n == 2 * rows * (1 + RS) + (N * nvis + 255) // 256          # ... and by the library's own workspace size
    img, A = place(inp['images'], dev, p.get('shift_img', 0)), place(inp['A'], dev, p.get('shift_A', 0))
    tgt, sig = place(inp['target'], dev), place(inp['sigma'], dev)
    wide = R % 2 == 0 and A.data_ptr() % 16 == 0 and img.data_ptr() % 8 == 0
    assert wide == (R % 2 == 0 and not p.get('shift_img') and not p.get('shift_A'))
    code = {'vis': 0, 'amp': 1, 'cphase': 2}[p['dtype']]
    grad = p.get('grad', True)

    def run():
        ws, loss = Out(ws_n, dev), Out(1, dev)
        dimg = Out(N * R, dev, p.get('shift_img', 0)) if grad else None
        rc = lib.bhn_chi2_eht(ptr(img), ptr(A), ptr(tgt), ptr(sig), inp['scale'], code, N, C_, nvis, R, ptr(ws.view), ptr(loss.view),
                              ptr(dimg.view) if dimg else None, _stream(dev))
        assert rc == BHN_OK, lib.bhn_last_error()
        torch.cuda.synchronize(dev)
        ws.numpy()
        out = dict(loss0=loss.numpy().reshape(()))
        if dimg:
            out['dimg'] = dimg.numpy().reshape(N, R)
        return out
    judge(case, inp, twice(run))


def _fov(ext):
    return (C.c_float * 3)(*[float(v) for v in ext])


@pytest.mark.parametrize('case', ids('trilinear'))
def test_trilinear(dev, lib, case):
    inp, p = sc.inputs(case), case.p
    N, sh = p['N'], p.get('shift', 0)
    pts, grid = place(inp['points'], dev, sh), place(inp['grid'], dev, sh)
    nx, ny, nz = p['n']

    def run():
        out = Out(N, dev, sh)
        rc = lib.bhn_trilinear(ptr(pts), N, ptr(grid), nx, ny, nz, _fov(inp['ext']), ptr(out.view), _stream(dev))
        assert rc == BHN_OK, lib.bhn_last_error()
        torch.cuda.synchronize(dev)
        return dict(out=out.numpy())
    judge(case, inp, twice(run))


def _geometry(inp, p, dev, with_dom):
    from bhnerf_amd import _hip
    keep = {k: place(inp[k], dev) for k in ('x', 'y', 'z', 'Omega', 't_geo', 'w', 'tM0')}
    if with_dom:
        keep['dom'] = place(inp['dom'], dev)
    geom = _hip.bhn_geom(R=p['R'], G=p['G'], S=p['S'], x=keep['x'].data_ptr(), y=keep['y'].data_ptr(), z=keep['z'].data_ptr(),
                         Omega=keep['Omega'].data_ptr(), t_geo=keep['t_geo'].data_ptr(), w=keep['w'].data_ptr(),
                         dom=keep['dom'].data_ptr() if with_dom else None)
    frames = _hip.bhn_frames(B=p['B'], tM0=keep['tM0'].data_ptr(), clock_probe=None)
    return geom, frames, keep


@pytest.mark.parametrize('case', ids('voxel'))
def test_voxel_render(dev, lib, case):
    inp, p = sc.inputs(case), case.p
    B, R, Sx = p['B'], p['R'], max(p['S'], 1)
    geom, frames, keep = _geometry(inp, p, dev, False)
    grid = place(inp['grid'], dev)
    nx, ny, nz = p['n']
    stride = nx * ny * nz if p['per_frame'] else 0

    def run():
        images = Out(B * Sx * R, dev)
        rc = lib.bhn_voxel_render_fwd(C.byref(geom), C.byref(frames), ptr(grid), nx, ny, nz, stride, _fov(inp['ext']), ptr(images.view), _stream(dev))
        assert rc == BHN_OK, lib.bhn_last_error()
        torch.cuda.synchronize(dev)
        return dict(images=images.numpy().reshape(B, Sx, R))
    judge(case, inp, twice(run))


@pytest.mark.parametrize('case', ids('grid'))
def test_grid_predictor_forward_and_backward(dev, lib, case):
    inp, p = sc.inputs(case), case.p
    B, R, G, Sx, res = p['B'], p['R'], p['G'], max(p['S'], 1), p['res']
    geom, frames, keep = _geometry(inp, p, dev, True)
    grid, dimg = place(inp['grid'], dev), place(inp['dimg'], dev)
    args = (C.byref(geom), C.byref(frames), ptr(grid), res, inp['scale'])

    def forward():
        emission, images = Out(B * R * G, dev), Out(B * Sx * R, dev)
        assert lib.bhn_grid_predict_fwd(*args, ptr(emission.view), _stream(dev)) == BHN_OK, lib.bhn_last_error()
        assert lib.bhn_grid_render_fwd(*args, ptr(images.view), _stream(dev)) == BHN_OK, lib.bhn_last_error()
        torch.cuda.synchronize(dev)
        return dict(emission=emission.numpy().reshape(B, R * G), images=images.numpy().reshape(B, Sx, R))
    got = twice(forward)
    dgrid = Out(res ** 3, dev)                              # holds the sentinel: the call itself must zero it (float atomics: run once)
    assert lib.bhn_grid_render_bwd(*args, ptr(dimg), ptr(dgrid.view), _stream(dev)) == BHN_OK, lib.bhn_last_error()
    torch.cuda.synchronize(dev)
    got['dgrid'] = dgrid.numpy().reshape(res, res, res)
    judge(case, inp, got)


def test_documented_refusals_return_their_code_without_launching(dev, lib):
    """G = 1025; C = 0 or 9 for cphase; C = 2 for vis; res = 1; S = 5; a non-positive extent: BHN_EINVAL, outputs untouched."""
    one = place(np.ones(8 * 1025, dtype=np.float32), dev)
    out = Out(4096, dev)
    st = _stream(dev)
    seen = []

    def refused(name, rc):
        torch.cuda.synchronize(dev)
        assert rc == BHN_EINVAL and out.untouched() and lib.bhn_last_error(), name
        seen.append(name)
    refused('rt_G1025', lib.bhn_radiative_transfer_fwd(ptr(one), ptr(one), ptr(one), ptr(one), ptr(out.view), 1, 1, 1025, st))
    refused('rt_G1025', lib.bhn_radiative_transfer_bwd(ptr(one), ptr(one), ptr(one), ptr(one), ptr(out.view), 1, 1, 1025, st))
    eht = lambda code, C_: lib.bhn_chi2_eht(ptr(one), ptr(one), ptr(one), ptr(one), 1.0, code, 1, C_, 2, 16, ptr(out.view[64:]), ptr(out.view), ptr(out.view[8:]), st)
    refused('cphase_C0', eht(2, 0))
    refused('cphase_C9', eht(2, 9))
    refused('vis_C2', eht(0, 2))
    refused('vis_C2', eht(1, 2))
    case = sc.BY_FAMILY['grid'][0]
    inp = sc.inputs(case)
    geom, frames, keep = _geometry(inp, case.p, dev, True)
    grid = place(inp['grid'], dev)
    for fn in (lib.bhn_grid_predict_fwd, lib.bhn_grid_render_fwd):
        refused('grid_res1', fn(C.byref(geom), C.byref(frames), ptr(grid), 1, 4.0, ptr(out.view), st))
    refused('grid_res1', lib.bhn_grid_render_bwd(C.byref(geom), C.byref(frames), ptr(grid), 1, 4.0, ptr(one), ptr(out.view), st))
    ext = _fov((8.0, 8.0, 8.0))
    refused('voxel_extent0', lib.bhn_voxel_render_fwd(C.byref(geom), C.byref(frames), ptr(grid), 5, 5, 5, 0, _fov((8.0, 0.0, 8.0)), ptr(out.view), st))
    refused('trilinear_extent_neg', lib.bhn_trilinear(ptr(one), 4, ptr(grid), 5, 5, 5, _fov((8.0, 8.0, -1.0)), ptr(out.view), st))
    geom.S = 5
    refused('grid_S5', lib.bhn_grid_render_fwd(C.byref(geom), C.byref(frames), ptr(grid), 5, 4.0, ptr(out.view), st))
    refused('voxel_S5', lib.bhn_voxel_render_fwd(C.byref(geom), C.byref(frames), ptr(grid), 5, 5, 5, 0, ext, ptr(out.view), st))
    refused('geom_S5', lib.bhn_geom_prepare(ptr(one), ptr(one), ptr(one), ptr(one), ptr(one), 5, 4, 1.0, 2.0, 3.0, ptr(out.view), ptr(out.view[16:]), st))
    assert set(seen) == set(sc.REFUSALS)
