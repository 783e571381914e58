"""CPU checks of what test_gpu_buffer_contract stands on: the case table's ray sets are what it says they are, every case's float64
reference is non-zero in every tensor, the problem builder factored out of frame_chunk_cases still draws the frame-chunk problems bit
for bit, the fill bytes decode as the GPU module says, and (host-only bhn_tape_info) every case takes the path it is listed under."""
import numpy as np
import pytest
import torch

import buffer_contract_cases as bc
import frame_chunk_cases as fc
from conftest import mask_tie_points
from gpu_support import expected_flags
from mlp_problems import problem_checksum, tensor_cuts
from oracle import oracle_np as onp

# sha256 (first 16 hex digits) of every frame_chunk_cases problem as the builder drew it BEFORE build_problem was factored out of
# problem() (mlp_problems.problem_checksum, run on the parent commit's module)
PINNED = {
    '4x128 S0 dense 144': 'c82d0a40658659db',
    '4x128 S3 compacted': '4771f6dfb7cd9de7',
    '4x100 S2 dense 96': '98cfd6a3836233f8',
    '4x256 S0 dense 144': '10400f37d11a1b9b',
    '4x256 S3 dense 96': 'e5e26d99a79b1e4f',
    '6x256 S1 compacted': 'ab81011152b99b91',
    '2x256 S0 dense 96': 'e808fb441fea6b2b',
    '6x64 S2 dense 144': 'd0a7c0ee6a3e0b6c',
    '6x128 S0 dense 96': 'd28ee4c55ebeed96',
    '4x256 f32 S3 dense 144': '708830c8f2085e65',
    '4x64 f32 S0 dense 96': '77501f7952377b39',
    '8x32 f32 S0 dense 96': '7481d6f9bbeedf53',
    '4x256 f32 S4 dense 96': 'ab1775e35b924085',       # (added with its V row; it has no earlier draw)
    '4x128 S0 dense 96': '380f785ce029706e',
    '4x256 S0 dense 96': 'f5a037d7b2511d6f',
}


def test_builder_reproduces_the_frame_chunk_problems_bit_for_bit():
    assert set(PINNED) == set(fc.CASES) | set(fc.STEP_CASES)
    for name, want in PINNED.items():
        assert problem_checksum(fc.problem(name)) == want, name


def test_case_table_ray_sets():
    bc.check_table()
    # one case per backward path, each ray set used
    assert {c[6] for c in bc.CASES.values()} == {'fused128', 'ga0_chain', 'fold', 'generic', 'f32', 't8', 'general', 'general f32'}
    assert {c[5] for c in bc.CASES.values()} == set(bc.RAY_SETS)


@pytest.mark.parametrize('name', list(bc.CASES))
def test_problem_has_no_mask_ties_and_pre_injection_samples(name):
    prob = bc.problem(name)
    g = prob['g']
    assert int(g['hparams'][4]) == bc.CASES[name][4] and g['kernel0'].shape[0] == 3 + 6 * bc.CASES[name][4]
    assert not mask_tie_points(g).any()
    tM = g['t_frames'].reshape(-1, 1, 1, 1) / onp.GM_C3_SGRA_HR + g['t_geos'] - fc.T_INJ
    pre = (tM < 0).sum(axis=(1, 2, 3))
    assert len(g['t_frames']) == 3 and 0 < pre[0] < tM[0].size and pre[-1] < pre[0]
    if prob['rays'].startswith('compacted'):
        # pre-injection samples INSIDE the domain too (the compacted layout holds only those)
        assert 0 < ((tM[0] < 0) & bc.domain_mask(prob)).sum() < bc.domain_mask(prob).sum()


@pytest.mark.parametrize('name', list(bc.CASES))
def test_float64_reference_is_nonzero_in_every_tensor(name):
    prob = bc.problem(name)
    ref = bc.reference(name)
    assert np.isfinite(ref['images']).all() and (np.abs(ref['images']).reshape(-1, ref['images'].shape[-1]).max(axis=1) > 0).all()   # every frame and plane
    assert (ref['emission'] != 0).any(axis=1).all()
    cuts = tensor_cuts(prob['g'])
    assert cuts[-1] == ref['grad'].size and np.isfinite(ref['grad']).all()
    for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
        assert np.abs(ref['grad'][c0:c1]).max() > 0, (name, 'tensor %d' % i)


def test_fill_bytes_decode_as_stated():
    """0xFF: NaN as f32 and as bf16, every bit set; 0x7F: 3.39e38 as f32, the same magnitude as bf16 (both finite)."""
    ff = torch.full((8,), 0xFF, dtype=torch.uint8)
    assert torch.isnan(ff.view(torch.float32)).all() and torch.isnan(ff.view(torch.bfloat16).float()).all()
    assert (ff.view(torch.int32) == -1).all()
    s7 = torch.full((8,), 0x7F, dtype=torch.uint8)
    f, b = s7.view(torch.float32), s7.view(torch.bfloat16).float()
    assert torch.isfinite(f).all() and torch.isfinite(b).all()
    assert abs(float(f[0]) / 3.39e38 - 1) < 2e-3 and abs(float(b[0]) / 3.39e38 - 1) < 2e-3
    z = torch.zeros((8,), dtype=torch.uint8)
    assert (z.view(torch.float32) == 0).all() and (z.view(torch.bfloat16).float() == 0).all()
    # e4m3 (OCP, no infinities): exponent and mantissa all ones = NaN, with either sign bit
    for byte in (0xFF, 0x7F):
        assert (byte >> 3) & 0xF == 0xF and byte & 0x7 == 0x7


def tape_info(depth, width, deg, mode, groups):
    from bhnerf_amd import engine
    eng = engine.FusedPredictor.__new__(engine.FusedPredictor)        # (host-only query: no device, no buffers)
    from bhnerf_amd import _hip
    eng.mode = _hip.MODES[mode]
    eng.model = _hip.make_model(depth, width, deg, True, 8.0, 0.0, np.inf, np.inf)
    return eng.tape_info(groups)


@pytest.mark.parametrize('name', list(bc.CASES))
def test_case_takes_the_path_it_is_listed_under(name):
    depth, width, mode, S, deg, rays, recipe, nwf = bc.CASES[name]
    info = tape_info(depth, width, deg, mode, bc.ragged_properties(name)[1])
    for k, v in expected_flags(recipe).items():
        assert info['flags'][k] == v, (name, k, info['flags'])
    assert info['fwd_groups_per_tile'] == nwf, (name, info)


def test_x12_is_the_smallest_such_ray_set():
    """No smaller dense set of 50-sample rays has 12-group tiles AND a group count that is no multiple of 12."""
    rays = bc.RAY_SETS['x12'][0] * bc.RAY_SETS['x12'][1]
    groups = lambda r: (50 * r + 31) // 32
    assert tape_info(4, 128, 3, 'bf16', groups(rays))['fwd_groups_per_tile'] == 12 and groups(rays) % 12 != 0
    for r in range(1, rays):
        assert tape_info(4, 128, 3, 'bf16', groups(r))['fwd_groups_per_tile'] == 8 or groups(r) % 12 == 0, r
