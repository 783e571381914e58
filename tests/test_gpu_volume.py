"""GPU tests of bhn_volume_render (bhnerf_amd/csrc/volume_render.hip) and VolumeVisualizer.render.

The cases, their inputs, the float64 restatement and the bound live in tests/volume_cases.py; tests/test_volume_refs_cpu.py proves
on the CPU that the restatement is the reference's arithmetic and that each case sees its slips at >= 5x the bound.  Here every case
goes through the C ABI twice into fresh outputs with sentinel guard bands: bitwise-equal results within the bound of the float64
restatement of the float32-rounded arrays (the view is double on both sides).  `observed / bound` is printed per case.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gpu_support
import volume_cases as vc
from gpu_support import dev, lib, place, ptr, stream_ptr as _stream  # noqa: F401

pytestmark = pytest.mark.gpu

BHN_OK, BHN_EINVAL = 0, 1


Out = functools.partial(gpu_support.Out, guard=vc.GUARD, sentinel=vc.SENTINEL)


def make_view(inp):
    from bhnerf_amd import _hip
    return _hip.bhn_volume_view(inp['fw'], inp['lw'], inp['bh'], (C.c_double * 3)(*inp['albedo']))


def run_abi(lib, dev, inp, shift=0, pad=0):
    """One call through the C ABI into a fresh guarded output: images (N, H, W, 3) float32."""
    N, H, W, S = inp['N'], inp['H'], inp['W'], inp['S']
    stride = H * W * S + pad
    em = np.full((N, stride), 7.5, dtype=np.float32)                # the padding between frames holds a large emission
    em[:, :H * W * S] = inp['emission'].reshape(N, -1)
    d = dict(pts=place(inp['pts'], dev, shift), em=place(em, dev, shift), sc=place(inp['alpha_scale'], dev, shift), lut=place(inp['lut'], dev, shift))
    view = make_view(inp)
    out = Out(N * H * W * 3, dev, shift)
    rc = lib.bhn_volume_render(ptr(d['pts']), ptr(d['em']), ptr(d['sc']), N, H, W, S, stride, ptr(d['lut']), len(inp['lut']), C.byref(view),
                               ptr(out.view), _stream(dev))
    assert rc == BHN_OK, lib.bhn_last_error()
    torch.cuda.synchronize(dev)
    return out.numpy().reshape(N, H, W, 3)


@pytest.mark.parametrize('case', [pytest.param(c, id=c.name) for c in vc.CASES])
def test_case_through_the_abi_twice_bitwise_equal_and_within_the_bound(dev, lib, case):
    inp = vc.inputs(case)
    a = run_abi(lib, dev, inp, case.p['shift'], case.p['pad'])
    b = run_abi(lib, dev, inp, case.p['shift'], case.p['pad'])
    assert a.tobytes() == b.tobytes()
    ref = vc.reference(case, inp)
    err = vc.error(a, ref)
    print(vc.report(case, err))
    assert np.isfinite(a).all() and err <= vc.BOUND, vc.report(case, err)
    if case.p.get('exact_one'):
        assert (a == 1.0).all()                                     # rays that miss the cube: exactly the white background


def test_documented_refusals_return_einval_and_leave_the_output_untouched(dev, lib):
    from bhnerf_amd import _hip
    inp = vc.inputs(next(c for c in vc.CASES if c.name == 'S20_lpr32'))
    N, H, W, S = inp['N'], inp['H'], inp['W'], inp['S']
    d = dict(pts=place(inp['pts'], dev), em=place(inp['emission'], dev), sc=place(inp['alpha_scale'], dev), lut=place(inp['lut'], dev))
    out = Out(N * H * W * 3, dev)
    seen = []

    def call(name, **over):
        a = dict(pts=ptr(d['pts']), em=ptr(d['em']), sc=ptr(d['sc']), N=N, H=H, W=W, S=S, lut=ptr(d['lut']), lut_n=len(inp['lut']),
                 view=C.byref(make_view(inp)), images=ptr(out.view))
        a.update(over)
        rc = lib.bhn_volume_render(a['pts'], a['em'], a['sc'], a['N'], a['H'], a['W'], a['S'], H * W * S, a['lut'], a['lut_n'], a['view'], a['images'], _stream(dev))
        torch.cuda.synchronize(dev)
        assert rc == BHN_EINVAL and out.untouched() and lib.bhn_last_error(), name
        seen.append(name)

    def view(**kw):
        v = dict(fw=inp['fw'], lw=inp['lw'], bh=inp['bh'])
        v.update(kw)
        return C.byref(_hip.bhn_volume_view(v['fw'], v['lw'], v['bh'], (C.c_double * 3)(0, 0, 0)))
    call('null_pts', pts=None); call('null_emission', em=None); call('null_scale', sc=None); call('null_lut', lut=None)
    call('null_view', view=None); call('null_images', images=None)
    call('N0', N=0); call('H0', H=0); call('W0', W=-1); call('S0', S=0); call('lut_n1', lut_n=1)
    call('facewidth0', view=view(fw=0.0)); call('linewidth0', view=view(lw=-0.1)); call('bh_negative', view=view(bh=-1.0))
    assert seen == vc.REFUSALS


@pytest.mark.parametrize('name', ['a', 'b'])
def test_visualizer_meets_the_golden_image(dev, name):
    """set_view -> render through Python on the golden view: the reference's own image, within the bound."""
    from bhnerf_amd import visualization
    g = vc.golden()
    domain_r, cam_r, fw, lw, bh = (float(v) for v in g['params'][:5])
    W, H, S, az, zen = g['view_' + name]
    viz = visualization.VolumeVisualizer(int(W), int(H), int(S))
    viz.set_view(cam_r, domain_r, az, zen)
    assert np.array_equal(viz._pts.astype(np.float32), g['pts_' + name])           # the float32 points the golden images belong to
    e = g['emission_' + name]
    for key, kw in (('nobh', {}), ('bh', dict(bh_radius=bh, bh_albedo=list(g['params'][5:8])))):
        img = viz.render(e, fw, linewidth=lw, cmap='hot', **kw)
        assert isinstance(img, np.ndarray) and img.shape == (int(H), int(W), 3)
        err = vc.error(img, g['image_%s_%s' % (name, key)])
        print('golden %s %s: %.2e / %.0e' % (name, key, err, vc.BOUND))
        assert err <= vc.BOUND
    lut = g['lut_hot']
    again = viz.render(torch.as_tensor(e, device=dev), fw, jit=True, linewidth=lw, cmap=np.concatenate([lut, np.ones((256, 1))], axis=1))
    assert isinstance(again, torch.Tensor) and again.is_cuda
    assert again.cpu().numpy().tobytes() == viz.render(e, fw, linewidth=lw, cmap='hot').tobytes()      # the (n, 4) array form is the named table


def test_frames_in_one_launch_equal_single_calls_bitwise(dev):
    from bhnerf_amd import visualization
    case = next(c for c in vc.CASES if c.name == 'N6_two_groups')
    inp = vc.inputs(case)
    viz = visualization.VolumeVisualizer(inp['W'], inp['H'], inp['S'])
    viz._pts = inp['pts'].astype(np.float64)                         # the case's points in place of a camera's
    movie = viz.render(inp['emission'], inp['fw'], linewidth=inp['lw'], cmap=inp['lut'])
    assert movie.shape == (inp['N'], inp['H'], inp['W'], 3)
    for n in range(inp['N']):
        one = viz.render(inp['emission'][n], inp['fw'], linewidth=inp['lw'], cmap=inp['lut'])
        assert one.shape == (inp['H'], inp['W'], 3) and one.tobytes() == movie[n].tobytes(), n
    assert vc.error(movie, vc.reference(case, inp)) <= vc.BOUND       # each frame normalised by its own maximum
    # an all-zero frame: alpha scale 0 (the reference divides by amax = 0), finite image, the wireframe alone
    e = inp['emission'].copy()
    e[1] = 0.0
    img = viz.render(e, inp['fw'], linewidth=inp['lw'], cmap=inp['lut'])
    assert np.isfinite(img).all() and img[0].tobytes() == movie[0].tobytes()


def test_network_to_render_end_to_end(dev, lib):
    """network.sample_3d_grid(predictor.apply, params, coords=visualizer.coords) -> render on a 4x128 network at 8 x 6 x 16: the
    image is the kernel's, called through the ABI on the same sampled emission."""
    from bhnerf_amd import network, visualization
    from oracle import oracle_np as onp
    viz = visualization.VolumeVisualizer(8, 6, 16)
    viz.set_view(37.0, 8.0, 0.4, 1.0)
    predictor = network.NeRF_Predictor(8.0, 2.0, 8.0, 4.0, net_depth=4, net_width=128, mode='f32', device=dev)
    tree = onp.he_uniform_params(np.random.default_rng(5), 4, 128, 21)
    tree['MLP_0']['Dense_4']['bias'] = tree['MLP_0']['Dense_4']['bias'] + 10.0        # sigmoid(out - 10): emission of order 0.5
    emission = network.sample_3d_grid(predictor.apply, network.ParamTree(tree), coords=viz.coords)
    assert emission.shape == (6, 8, 16) and emission.max() > 0.05
    img = viz.render(emission, 15.2, bh_radius=2.0, bh_albedo=[0.5, 0.5, 0.5])
    e32 = np.ascontiguousarray(emission, dtype=np.float32)
    inp = dict(pts=viz._pts.astype(np.float32), emission=e32[None], alpha_scale=(np.float32(1.0) / e32.max(keepdims=True).reshape(1)).astype(np.float32),
               lut=visualization._colour_table('hot'), fw=15.2, lw=0.1, bh=2.0, albedo=(0.5, 0.5, 0.5), N=1, H=6, W=8, S=16)
    direct = run_abi(lib, dev, inp)[0]
    assert img.shape == (6, 8, 3) and img.tobytes() == direct.tobytes()
    ref = vc.render_ref(inp['pts'], inp['emission'], inp['alpha_scale'], inp['lut'], inp['fw'], inp['lw'], inp['bh'], inp['albedo'])[0]
    assert vc.error(img, ref) <= vc.BOUND and np.abs(ref - 1.0).max() > 0.05        # not just the background
