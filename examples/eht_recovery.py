"""Recovery of 3-D emission from EHT observations end to end on one MI355X (the flow of the reference's Tutorial 4, with its
Tutorial 2 inside), with nothing but this package -- no ehtim, no astropy:

  Kerr geodesics (own tracer)  ->  a Gaussian hotspot on a Keplerian orbit  ->  image_plane_dynamics: the 'true' movie  ->
  empty_eht_obs: the (u, v) tracks, elevations and thermal noise of a station table (ngEHT, GMST 2 h + 40 min, 64 frames)  ->
  observe_same: noisy complex visibilities  ->  TrainStep.eht_obs on 'vis', 'amp', 'cphase', 'logcamp' or a '+'-joined set  ->
  Optimizer.run  ->  the 3-D emission sampled back.

    python examples/eht_recovery.py [--dtype vis] [--array ngEHT] [--size 32] [--iters 1000] [--render out] [--tracer hip]
    python examples/eht_recovery.py --stokes --gains          # a polarised movie behind unknown station gains
    python examples/eht_recovery.py --tv 1e3 [--tv-res 32]    # the data term plus a total-variation prior on the emission volume
    python examples/eht_recovery.py --tv 1e3 --joint          # the same objective, ONE Adam step per iteration on the summed gradient

--stokes observes a polarised movie (Stokes I, Q, U through the transported factors J of a vertical field) and fits what station
gains cannot touch: TrainStep.eht_obs(.., 'cphase+logcamp') on the I plane (the Q and U planes of its data get sigma = +inf) plus
TrainStep.eht_obs(.., 'm'), the visibility-domain fractional polarisation (Q~ + iU~) / I~ -- two losses, a render and an Adam step
each (TrainStep.__add__).  The same data are then fitted on the calibrated 'vis' of the three planes for contrast.  --gains
corrupts the clean visibilities with random complex station gains (observation.station_gains: 10 % amplitudes, random phases,
common to the Stokes planes) before the thermal noise: the first fit does not see them, the second fits them as if they were sky.
--array names a table under tests/golden/eht_arrays/ (ngEHT, EHT2017) or is the path of one in the same text format.
--render PATH also renders the recovered volume through visualization.VolumeVisualizer and saves PATH.npy (PATH.png with
matplotlib).  --tv W adds TrainStep.volume_prior (the smoothed total variation of the emission on a --tv-res^3 lattice over the
field of view, a mean over the in-domain voxels, times W) to whatever objective the flags select: a second loss with a render of
the lattice and an Adam step of its own.  The chi^2 printed is the data term's alone, and every fit ends with the tv of the
recovered 64^3 volume (engine.chi2_volume as a metric), so that runs with and without the prior compare.  --joint builds every
sum above with TrainStep.joint instead of +: one render of the ray set for all terms on it, the terms' gradients summed, one Adam
step per iteration -- the form in which the weight of --tv acts against the data term.  What is and is not ehtim here: see observation.empty_eht_obs and INTEGRATION.md.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bhnerf_amd as bhnerf  # noqa: E402
from bhnerf_amd import constants, kgeo, network, observation, optimization, units  # noqa: E402

# GM / c^2 of Sgr A* over its distance (26673 light years), in radians: 5.0 micro-arcseconds
RAD_PER_M = constants.GM_c3('s') * 299792458.0 / (26673 * 9.4607304725808e15)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='vis', help="'vis', 'amp', 'cphase', 'logcamp' or a '+'-joined set such as 'cphase+logcamp'")
    ap.add_argument('--array', default='ngEHT', help='a table under tests/golden/eht_arrays/ or the path of one')
    ap.add_argument('--size', type=int, default=32, help='image is size x size pixels')
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--render', metavar='PATH', default=None, help='render the recovered volume to PATH.npy (and PATH.png with matplotlib)')
    ap.add_argument('--ngeo', type=int, default=64)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--width', type=int, default=128)
    ap.add_argument('--mode', default='bf16', choices=['bf16', 'f32'], help='arithmetic of the fused kernels')
    ap.add_argument('--batch', type=int, default=6, help='frames per step')
    ap.add_argument('--count', default='min', choices=['min', 'max'], help='closure sets per frame: an independent set or all')
    ap.add_argument('--seed', type=int, default=0, help='seed of the thermal noise')
    ap.add_argument('--tracer', default='numpy', choices=['numpy', 'hip'], help='where the geodesics are integrated: on the host or on the GPU')
    ap.add_argument('--stokes', action='store_true', help="a polarised movie (I, Q, U): fit 'cphase+logcamp' on I plus 'm', then 'vis' for contrast")
    ap.add_argument('--gains', action='store_true', help='corrupt the visibilities with random complex station gains (seed: --seed + 1)')
    ap.add_argument('--tv', type=float, default=0.0, metavar='W', help='weight of a total-variation prior on the emission volume (0: none)')
    ap.add_argument('--joint', action='store_true', help='one Adam step on the summed gradient of the terms (TrainStep.joint) where the default '
                    'lets every term take a step of its own (+): the weight of --tv then acts against the data term')
    ap.add_argument('--tv-res', type=int, default=32, metavar='N', help='the prior samples the emission on an N x N x N lattice over the field of view')
    args = ap.parse_args()

    fov_M, spin, inclination, nt = 16.0, 0.2, np.deg2rad(60.0), args.frames
    flux_scale = 0.1                                            # image-plane fluxes of a `reasonable` size in Jy
    tstart = 2.0                                                # GMST hours
    tstop = tstart + 40.0 / 60.0
    rmax, z_width = fov_M / 2, 4.0

    geos = kgeo.image_plane_geos(spin, inclination, (-fov_M / 2, fov_M / 2), (-fov_M / 2, fov_M / 2), ngeo=args.ngeo,
                                 num_alpha=args.size, num_beta=args.size, backend=args.tracer)
    Omega = np.sign(spin + np.finfo(float).eps) / (np.asarray(geos.r) ** 1.5 + spin)           # Keplerian, prograde (M = 1)
    geos['g'] = kgeo.doppler_factor(geos, kgeo.azimuthal_velocity_vector(geos, Omega))
    t_injection = -float(geos.r_o)
    emission_0 = flux_scale * np.asarray(bhnerf.emission.generate_hotspot_xr(
        resolution=(64, 64, 64), rot_axis=[0.0, 0.0, 1.0], rot_angle=0.0, orbit_radius=5.5, std=0.7, r_isco=constants.isco_pro(spin),
        fov=(fov_M, 'GM/c^2')).data)
    t_frames = np.linspace(tstart, tstop, nt) * units.hr
    rmin = float(np.asarray(geos.r).min())
    J = 1.0
    if args.stokes:       # transported Stokes factors [I, Q, U] of a vertical field; the I factor of unit mean over the recovery domain,
        #                   so that the fluxes are of the unpolarised movie's size
        J = np.nan_to_num(kgeo.emission_factors(geos, Omega, dict(arad=0.0, avert=1.0, ator=0.0), V_frac=0.0)[1], nan=0.0)
        inside = (np.nan_to_num(np.asarray(geos.r), nan=np.inf) < rmax) & (np.abs(np.nan_to_num(np.asarray(geos.z))) < z_width) & (J[0] > 0)
        J = J / J[0][inside].mean()
    movie = bhnerf.emission.image_plane_dynamics((emission_0, fov_M), geos, Omega, t_frames, t_injection, J=J, doppler=True)

    # Tutorial 2: the empty observation of the station table and the synthetic data.  The scans sit at the movie's frame times.
    path = args.array if os.path.exists(args.array) else os.path.join(ROOT, 'tests', 'golden', 'eht_arrays', args.array + '.txt')
    obs_params = {'mjd': 57851, 'timetype': 'GMST', 'nt': nt, 'tstart': tstart, 'tstop': tstop, 'tint': 30.0,
                  'array': observation.Array.load_txt(path)}
    obs = observation.empty_eht_obs(times=np.linspace(tstart, tstop, nt), **obs_params)
    fov_rad = fov_M * RAD_PER_M
    gains = observation.station_gains(obs, seed=args.seed + 1) if args.gains else None
    vis = observation.observe_same(movie, obs, fov_rad, thermal_noise=True, seed=args.seed, gains=gains)
    up = obs.up[0].sum()
    snr = np.abs(vis[:, 0] if args.stokes else vis)[obs.up] / obs.sigma[obs.up]
    flux = (movie[:, 0] if args.stokes else movie).sum((-1, -2))                      # Stokes I
    print('%s: %d stations, %d of %d baselines up in frame 0, |uv| up to %.1f Glambda; movie %s of %.3g .. %.3g Jy, median SNR %.0f'
          % (os.path.basename(path), len(obs.array), up, obs.nvis, np.sqrt((obs.uv[obs.up] ** 2).sum(-1)).max() / 1e9, movie.shape,
             flux.min(), flux.max(), np.median(snr)))
    if args.gains:
        print('station gains: |G| %.2f .. %.2f, random phases, common to the Stokes planes' % (np.abs(gains).min(), np.abs(gains).max()))

    # Tutorial 4: the training step on the observation, the optimisation and the recovered volume
    rt = network.raytracing_args(geos, Omega, t_injection, t_frames[0], J=J)
    if not args.stokes:
        train_step = optimization.TrainStep.eht_obs(t_frames, obs, vis, fov_rad, args.size, dtype=args.dtype, count=args.count)
        fit(args, "'%s'" % args.dtype, train_step, geos, rt, rmin, rmax, z_width, fov_M, render=args.render)
        return
    # what the gains cannot touch: the closure quantities of Stokes I (the Q and U planes of that step carry no weight) plus 'm'
    data = obs.data(vis, 'cphase+logcamp', count=args.count)
    for term in ('cphase', 'logcamp'):
        data[term][1][:, 1:] = np.inf
    closure = optimization.TrainStep.eht_closure(t_frames, obs.uv, fov_rad, args.size, obs.pairs, {t: data[t] for t in ('cphase', 'logcamp')},
                                                 triangles=data['triangles'], quadrangles=data['quadrangles'])
    combine = optimization.TrainStep.joint if args.joint else (lambda a, b: a + b)
    robust = combine(closure, optimization.TrainStep.eht_obs(t_frames, obs, vis, fov_rad, args.size, dtype='m'))
    fit(args, "'cphase+logcamp' on I + 'm'", robust, geos, rt, rmin, rmax, z_width, fov_M, render=args.render)
    # for contrast: the calibrated visibilities of the three planes
    fit(args, "'vis'", optimization.TrainStep.eht_obs(t_frames, obs, vis, fov_rad, args.size, dtype='vis'), geos, rt, rmin, rmax, z_width, fov_M)


def fit(args, label, data_step, geos, rt, rmin, rmax, z_width, fov_M, render=None):
    """One optimisation from fresh parameters: chi^2 of the data before and after, the time per iteration, where the recovered
    emission peaks and its total variation."""
    import torch
    from bhnerf_amd import engine, regularization
    train_step = data_step
    if args.tv > 0:
        prior = optimization.TrainStep.volume_prior(fov_M, resolution=args.tv_res, weights={'tv': 1.0}, scale=args.tv)
        train_step = optimization.TrainStep.joint(data_step, prior) if args.joint else data_step + prior
        label += ' + %g tv at %d^3' % (args.tv, args.tv_res)
    if args.joint:
        label += ' (joint)'
    predictor = network.NeRF_Predictor(rmax, rmin, rmax, z_width, net_depth=4, net_width=args.width, mode=args.mode)
    opt = optimization.Optimizer({'num_iters': args.iters, 'lr_init': 1e-3, 'lr_final': 1e-4}, predictor, rt)
    first = optimization.total_movie_loss(args.batch, opt.state, data_step, rt)
    t0 = time.perf_counter()
    opt.run(args.batch, train_step, rt, log_fns=[optimization.LogFn(
        lambda o: print('iter %5d  chi2/frame %.4g' % (o.step, float(np.mean(o.loss)))), max(50, args.iters // 10))])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    last = optimization.total_movie_loss(args.batch, opt.state, data_step, rt)
    print('%s chi2 per frame %.4g -> %.4g   (%d iterations in %.1f s = %.2f ms/iteration)' % (label, first, last, args.iters, dt, 1e3 * dt / args.iters))
    n = 64
    ax = np.linspace(-rmax, rmax, n)
    vol = network.sample_3d_grid(predictor.apply, opt.state.params, fov=fov_M, resolution=n)
    i = np.unravel_index(np.argmax(vol), vol.shape)
    print('recovered emission peaks at (x, y, z) = (%.1f, %.1f, %.1f) M; truth (5.5, 0.0, 0.0) at the first frame' % (ax[i[0]], ax[i[1]], ax[i[2]]))
    # the prior as a metric: mean smoothed |grad e| over the recovery domain of the 64^3 volume
    x, y, z = np.meshgrid(ax, ax, ax, indexing='ij')
    r = np.sqrt(x ** 2 + y ** 2 + z ** 2)
    domain = ((r >= rmin) & (r <= rmax) & (np.abs(z) <= z_width)).astype(np.uint8)
    metric = regularization.VolumePrior(fov=fov_M, resolution=n, weights={'tv': 1.0})
    tv = engine.chi2_volume(torch.as_tensor(vol, device=opt.state.flat.device), metric, 1.0, mask=domain, want_grad=False)[0]
    print('tv of the recovered volume (mean |grad e| over %d in-domain voxels of %d^3): %.4e per M, peak emission %.4e' % (domain.sum(), n, float(tv), vol.max()))
    if render:
        from image_plane_recovery import render_volume
        render_volume(render, predictor, opt.state.params, rmax)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
