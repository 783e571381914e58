"""CPU checks of what test_gpu_general_path stands on: every case of general_path_cases has the property it is listed for, every branch
value of csrc/general_mlp.hip's host rules that the older suite never reached is reached by a case, the Python restatement of those rules
gives the sizes the library's host-only queries give, the problems are what they were when the table was written (sha256), and the two
conditions under which the GPU bounds mean something hold on the references alone: the ReLU-tie adjudication takes out at most a quarter
of a case's in-domain ray samples, and the emulator with float32 accumulation (accum32: the kernels' precision of accumulation, not
their order) moves a case by no more than a quarter of each cap of the bf16 comparison."""
import ctypes as C

import numpy as np
import pytest

import general_path_cases as gp
from general_path_cases import CASES, MODES, case_layout, problem, reference
from mlp_bounds import caps_of, expected_recipe, l2err, maxerr
from mlp_problems import problem_checksum, tensor_cuts

# sha256 (first 16 hex digits) of every problem as frame_chunk_cases.build_problem drew it when the table was written
PINNED = {
    '4x32 deg5 S0 ragged':            '93fa4dc96c936415',
    '3x96 deg6 S2 ragged':            'a0525d07eda7c3ef',
    '4x160 deg5 S3 compacted':        'e18c626ac2ab5133',
    '4x160 deg5 S0 noskip ragged':    'bee4c5fd8826614e',
    '6x224 deg7 S1 ragged':           '4494f0369f7d6ecc',
    '4x256 deg5 S2 ragged':           'f27a2a5c0ff949e9',
    '4x288 deg3 S2 ragged':           '79a7c2a202327709',
    '4x257 deg5 S0 ragged':           'b34b9b8e4bde2f19',
    '5x480 deg0 S2 tiny':             '89ee9b7968d156b3',
    '2x33 deg10 S3 tiny B1':          'dbc3d029dc344e20',
    '4x416 deg9 S1 compacted':        'ebe04039c2c41770',
    '4x128 deg5 S3 direct 64':        'dafe50c95b68d7d8',
    '4x320 deg6 S0 direct 64':        '52eb18fd0ac2a482',
    '4x128 deg5 S0 direct 33':        '5f8c0f02e6a1f9d7',
    '4x320 deg6 S2 long 257':         '590e0cb94894f423',
    '4x128 deg5 S2 compacted span2':  '3183fcd0401548b5',
    '4x128 deg5 S2 compacted 100':    '45165c070554131c',
}

# what each case is there for: values of case_layout (nt: the 32-column tiles of the strips of a hidden layer's weight-gradient jobs)
EXPECT = {
    '4x32 deg5 S0 ragged':            dict(MTp=1, waves=2, nt=[1], F=33, Ep=64, NG=4),
    '3x96 deg6 S2 ragged':            dict(MTp=3, waves=2, nt=[3], NG=4, skip=[False, False, True, True]),
    '4x160 deg5 S3 compacted':        dict(MTp=5, waves=4, nt=[4, 1], NG=4),
    '4x160 deg5 S0 noskip ragged':    dict(MTp=5, waves=4, nt=[4, 1], skip=[False] * 5),
    '6x224 deg7 S1 ragged':           dict(MTp=7, waves=4, nt=[4, 3], NG=4, skip=[False, False, False, False, True, False, False]),
    '4x256 deg5 S2 ragged':           dict(MTp=8, waves=8, block=512, NG=4, nsub=4, Ep=64),
    '4x288 deg3 S2 ragged':           dict(MTp=9, waves=8, nt=[4, 4, 1], NG=4, Ep=32, lds16=160288),
    '4x257 deg5 S0 ragged':           dict(MTp=9, waves=8, nt=[4, 4, 1], NG=2, Ep=64, F=33, Wp=288),
    '5x480 deg0 S2 tiny':             dict(MTp=15, waves=8, nt=[4, 4, 4, 3], NG=2, F=3, Ep=32, skip=[False, False, False, True, False, True]),
    '2x33 deg10 S3 tiny B1':          dict(MTp=2, Wp=64, F=63, Ep=64, total_tiles=1, skip=[False, False, True]),
    '4x416 deg9 S1 compacted':        dict(MTp=13, waves=8, nt=[4, 4, 4, 1], NG=2),
    '4x128 deg5 S3 direct 64':        dict(ray_direct=True, ray_span=None, NG=4),
    '4x320 deg6 S0 direct 64':        dict(ray_direct=True, ray_span=None, NG=2),
    '4x128 deg5 S0 direct 33':        dict(ray_direct=True, ray_span=None),
    '4x320 deg6 S2 long 257':         dict(ray_direct=False, ray_span=None, groups=73, NG=2),
    '4x128 deg5 S2 compacted span2':  dict(ray_direct=True, ray_span=2),
    '4x128 deg5 S2 compacted 100':    dict(ray_direct=False, ray_span=3),
}


def hidden_nt(L):
    return L['layers'][1]['nt']


def test_problems_are_drawn_bit_for_bit():
    assert set(PINNED) == set(CASES)
    for name, want in PINNED.items():
        assert problem_checksum(problem(name)) == want, name


@pytest.mark.parametrize('name', list(CASES))
def test_case_has_the_property_it_is_listed_for(name):
    depth, width, deg, S, rays, B, do_skip, _ = CASES[name]
    L = dict(case_layout(name), nt=hidden_nt(case_layout(name)), skip=gp.skip_inputs(depth, do_skip))
    for k, v in EXPECT[name].items():
        assert L[k] == v, (name, k, L[k], v)
    prob = problem(name)
    assert prob['B'] == B and len(prob['g']['t_frames']) == B and prob['g']['kernel0'].shape == (3 + 6 * deg, width)
    assert expected_recipe(depth, L['Wp'], general=True) == 'general'
    assert deg >= 5 or width > 256                                                  # (what sends a network down the general path)
    assert gp.points_per_frame(name) < 4000
    # the layers that take the encoded inputs are the ones whose kernels have the rows for them
    for l, s in enumerate(L['skip']):
        assert prob['g']['kernel%d' % l].shape[0] == (L['F'] if l == 0 else width + (L['F'] if s else 0)), (name, l)
        assert L['layers'][l]['erows'] == (L['Ep'] if l == 0 or s else 0)
    assert L['lds16'] <= 160 * 1024 and L['lds_f32'] <= 160 * 1024
    assert L['NG'] == 4 or L['lds16_at_4'] > 160 * 1024


def test_every_branch_value_the_older_suite_never_reached_is_reached():
    Ls = {n: case_layout(n) for n in CASES}
    have = lambda pred: [n for n, L in Ls.items() if pred(n, L)]
    # m-tiles per layer against the waves of a workgroup
    assert {L['MTp'] for L in Ls.values()} >= {1, 3, 5, 7, 8, 9, 13, 15}
    assert have(lambda n, L: L['MTp'] < L['waves']) and have(lambda n, L: L['MTp'] % L['waves'] not in (0, L['MTp']))
    assert have(lambda n, L: L['MTp'] == 8 and L['block'] == 512 and L['Wp'] == 256 and CASES[n][2] >= 5)
    # strips of the weight-gradient kernels: nt 1 and 3
    assert {L['Wp'] for L in Ls.values() if hidden_nt(L)[-1] == 1} >= {32, 160, 288, 416}
    assert {L['Wp'] for L in Ls.values() if hidden_nt(L)[-1] == 3} >= {96, 224, 480}
    # NG: both sides of the switch at the same width, the largest NG = 4 launch, NG = 4 on eight waves
    big = Ls['4x288 deg3 S2 ragged']
    assert big['NG'] == 4 and 159000 <= big['lds16'] <= 162000 and big['lds16'] == max(L['lds16'] for L in Ls.values() if L['NG'] == 4)
    assert have(lambda n, L: L['Wp'] == 288 and L['Ep'] == 64 and L['NG'] == 2)
    assert have(lambda n, L: L['Wp'] == 256 and L['Ep'] == 64 and L['NG'] == 4 and L['waves'] == 8 and L['nsub'] == 4 and CASES[n][2] > L['nsub'])
    # encoded inputs: no octave on a wide network; F = 33 and F = 63 together with a zero-padded width
    assert have(lambda n, L: CASES[n][2] == 0 and CASES[n][1] > 256)
    for F in (33, 63):
        assert have(lambda n, L: L['F'] == F and CASES[n][1] % 32 != 0 and L['Ep'] - F == 64 - F)
    # ... and that padded width on a layer that takes the encoded inputs behind the hidden ones (gen_reduce_kernel's row map)
        assert have(lambda n, L: L['F'] == F and CASES[n][1] % 32 != 0 and any(gp.skip_inputs(CASES[n][0], CASES[n][6])[1:]))
    # ray_direct: dense G = 64 and G <= 33, compacted ray_span <= 2; not direct: G = 257, ray_span 3
    G = lambda n: gp.RAY_SETS[CASES[n][4]][2]
    assert have(lambda n, L: L['ray_direct'] and L['ray_span'] is None and G(n) == 64)
    assert have(lambda n, L: L['ray_direct'] and L['ray_span'] is None and G(n) == 33)
    assert have(lambda n, L: L['ray_direct'] and L['ray_span'] == 2) and have(lambda n, L: not L['ray_direct'] and L['ray_span'] == 3)
    assert have(lambda n, L: not L['ray_direct'] and G(n) == 257)
    assert not gp.ray_direct(34) and gp.ray_direct(32) and not gp.ray_direct(96) and not gp.ray_direct(50) and not gp.ray_direct(50, 0)
    # chunks of the recomputing backward
    assert have(lambda n, L: L['total_tiles'] == 1)
    ng = set()
    for n in gp.CHUNK_SWEEP:
        L = Ls[n]
        total, tpf = L['total_tiles'], L['tiles_per_frame']
        ks = [total - 1 if k < 0 else k for k in gp.CHUNK_TILES]
        passes = {k: gp.chunks(total, k) for k in ks}
        assert all(sum(p[1] for p in ps) == total and not ps[0][2] and all(p[2] for p in ps[1:]) for ps in passes.values())
        for k in ks[1:3]:                                                                           # 3 and 5 tiles: passes that hold two frames
            assert tpf % k and any(gp.cuts_a_frame(p, tpf) for p in passes[k]), (n, k)
        assert total % 5 and any(gp.cuts_a_frame(p, tpf) for p in passes[5])                        # ... one of them does not divide the tile count
        assert any(ps[-1][1] < k for k, ps in passes.items()) and passes[total - 1][-1][1] == 1     # a short last chunk
        assert len(passes[2]) >= 3
        ng.add(L['NG'])
    assert ng == {2, 4} and any(CASES[n][4] == 'compacted' for n in gp.CHUNK_SWEEP)
    L = Ls['3x96 deg6 S2 ragged']
    assert L['NG'] == 4 and (L['tiles_per_frame'], L['total_tiles']) == (8, 24) and len(gp.chunks(24, 2)) == 12


def test_ray_sets():
    from bhnerf_amd import engine
    import torch
    for name in CASES:
        rays = CASES[name][4]
        H, Wd, G, dom = gp.RAY_SETS[rays]
        L = case_layout(name)
        if rays.startswith('compacted'):
            mask = gp.in_domain(name)
            n = int(mask.sum())
            assert 0 < n < 0.9 * H * Wd * G                                        # point-compacted by the engine
            ray = torch.from_numpy(np.repeat(np.arange(H * Wd), G)[mask.reshape(-1)])
            assert L['ray_span'] == gp.RAY_SPAN[rays] == engine.ray_span(ray), (name, L['ray_span'])
        else:
            assert L['groups'] == (H * Wd * G + 31) // 32 and L['ray_span'] is None
    assert case_layout('4x320 deg6 S2 long 257')['groups'] == 73 and gp.RAY_SETS['long 257'][0] * gp.RAY_SETS['long 257'][1] == 9
    # 257 samples: the longest ray that lies in at most two tiles of 8 x 32 points wherever it starts
    assert (255 + 257 - 1) // 256 == 1 and (255 + 258 - 1) // 256 == 2


@pytest.mark.parametrize('name', list(CASES))
def test_restated_layout_gives_the_sizes_of_the_library(name):
    """Host-only queries: the packed image and the workspace (slabs + tape) are what the restatement computes; the path is `general`."""
    from bhnerf_amd import _hip
    lib = _hip.lib()
    depth, width, deg, S, rays, B, do_skip, _ = CASES[name]
    L = case_layout(name)
    m = _hip.make_model(depth, width, deg, do_skip, *gp.RAY_SETS[rays][3])
    info = (C.c_int64 * _hip.BHN_TAPE_INFO_N)()
    for mode in MODES:
        assert int(lib.bhn_packed_bytes(C.byref(m), _hip.MODES[mode])) == L['packed_bytes'][mode], (name, mode)
        for nb, groups in ((B, L['groups']), (1, 16)):
            want = L['slab_bytes'] + nb * ((groups + 7) // 8) * 8 * L['tape_bytes'][mode]
            assert int(lib.bhn_render_bwd_workspace_bytes(C.byref(m), _hip.MODES[mode], nb, 32 * groups, 0)) == want, (name, mode, nb, groups)
        assert gp.workspace_bytes(name, mode, L['total_tiles']) == L['slab_bytes'] + L['total_tiles'] * 8 * L['tape_bytes'][mode]
        assert lib.bhn_tape_info(C.byref(m), _hip.MODES[mode], L['groups'], info, _hip.BHN_TAPE_INFO_N) == 0
        assert info[4] == _hip.TAPE_FLAGS['general']


@pytest.mark.parametrize('name', list(CASES))
def test_references_tie_share_and_accumulation_noise(name):
    """Both references are non-zero in every frame, plane and tensor; the tie adjudication would take out at most a quarter of the
    in-domain ray samples; float32 accumulation moves the emulator by at most a quarter of each cap."""
    prob = problem(name)
    cuts = tensor_cuts(prob['g'])
    dom = gp.in_domain(name) & (prob['g']['g'] != 0)
    for mode in MODES:
        ref = reference(name, mode)
        assert np.isfinite(ref['images']).all() and (np.abs(ref['images']).reshape(-1, ref['images'].shape[-1]).max(axis=1) > 0).all()
        assert (ref['emission'] != 0).any(axis=1).all() and cuts[-1] == ref['grad'].size and np.isfinite(ref['grad']).all()
        for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
            assert np.abs(ref['grad'][c0:c1]).max() > 0, (name, mode, 'tensor %d' % i)
        ties = reference(name, mode, want_ties=True) & dom
        assert 4 * int(ties.sum()) <= int(dom.sum()), (name, mode, int(ties.sum()), int(dom.sum()))
    ref, a32 = reference(name, 'bf16'), reference(name, 'bf16', accum32=True)
    cap = gp.bounds(name, 'bf16')
    fig = dict(image=maxerr(a32['images'], ref['images']), emission=l2err(a32['emission'], ref['emission']), grad=l2err(a32['grad'], ref['grad']),
               tensor=max(l2err(a32['grad'][c0:c1], ref['grad'][c0:c1]) for c0, c1 in zip(cuts[:-1], cuts[1:])))
    print('\n[general path] %-32s float32 accumulation moves the emulator by %s' % (name, '  '.join('%s %.2e (cap %.1e)' % (k, v, cap[k]) for k, v in fig.items())))
    caps = caps_of('random', CASES[name][2])           # (the emission has no cap of its own there: its figure is printed only)
    assert set(caps) == {'image', 'grad', 'tensor'} and all(cap[k] == v for k, v in caps.items())
    for k in caps:
        assert 4 * fig[k] <= caps[k], (name, k, fig[k], caps[k])
