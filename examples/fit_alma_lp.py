"""Polarised light-curve fit over an inclination grid -- the flow of the reference's scripts/Fit_ALMA_LP_Apr11_SgrA_Flare.py
(BASELINE config 5) with this package only:

  csv light curves -> alma.preprocess_data -> train / validation split in time -> for every inclination:
  alma.get_raytracing_args (own Kerr tracer, Doppler factor, parallel-transported polarisation) -> NeRF_Predictor +
  TrainStep.image(dtype='lc') + Optimizer with the SummaryWriter log hooks and checkpoints -> alma.chi2_df over the grid.

The ALMA data file does not ship with either repository: when `preprocess.data_path` is missing, a synthetic flare (an
orbiting Gaussian hotspot rendered through the same geometry at 30 deg, plus a constant shadow polarisation, Faraday
rotation and noise) is written there first.

    python examples/fit_alma_lp.py 20 30 40 [--config examples/fit_alma_lp.yaml] [--seeds 4] [--tracer hip] [--factors hip] [--resident]
"""
import argparse
import os
import sys

import numpy as np
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bhnerf_amd as bhnerf  # noqa: E402
from bhnerf_amd import units  # noqa: E402
from bhnerf_amd.optimization import LogFn  # noqa: E402


def synthetic_flare(path, model, pre, true_inc_deg=30.0, seed=0):
    """4-s cadence (I, Q, U) light curves of a hotspot on a Keplerian orbit, observed in three scans."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    scans = [(9.25, 9.95), (10.05, 10.75), (10.85, 11.75)]
    t = np.concatenate([np.arange(a, b, 4.0 / 3600.0) for a, b in scans])
    rt = bhnerf.alma.get_raytracing_args(np.deg2rad(true_inc_deg), model['spin'], model, rot_angle=np.deg2rad(pre['de_rot_angle'] + 20.0))[0]
    n, rmax = 48, model['fov_M'] / 2.0
    ax = np.linspace(-rmax, rmax, n)
    gx, gy, gz = np.meshgrid(ax, ax, ax, indexing='ij')
    hotspot = np.exp(-((gx - 11.0) ** 2 + gy ** 2 + gz ** 2) / (2 * 1.5 ** 2))
    geos = dict(x=rt['coords'][0], y=rt['coords'][1], z=rt['coords'][2], t=rt['t_geos'], dtau=rt['dtau'], Sigma=rt['Sigma'], g=rt['g'])
    coarse = t[::15]                                                               # render every minute, interpolate to the cadence
    movie = bhnerf.emission.image_plane_dynamics((hotspot, 2 * rmax), geos, rt['Omega'], coarse * units.hr, rt['t_injection'],
                                                 J=rt['J'], t_start_obs=rt['t_start_obs'])
    lc = movie.sum(axis=(-1, -2))
    lc *= pre['I_hs_mean'] / lc[:, 0].mean()
    iqu = np.stack([np.interp(t, coarse, lc[:, s]) for s in range(3)], axis=1)
    # what preprocess_data undoes: Faraday rotation and the constant shadow polarisation
    qu = bhnerf.emission.rotate_evpa(iqu[:, 1:], -np.deg2rad(pre['de_rot_angle']), axis=1)
    chi = np.deg2rad(pre['chi_sha'])
    qu = qu + pre['P_sha'] * np.array([np.cos(2 * chi), np.sin(2 * chi)]) + rng.normal(0.0, 5e-3, qu.shape)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    pd.DataFrame({'time': t, 'I': iqu[:, 0] + 2.4, 'Q': qu[:, 0], 'U': qu[:, 1]}).to_csv(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('inc', type=float, nargs='+', help='inclination angles [deg]')
    ap.add_argument('--seeds', type=int, nargs='+')
    ap.add_argument('--config', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fit_alma_lp.yaml'))
    ap.add_argument('--tracer', choices=['numpy', 'hip'], help="where the geodesics are integrated (default: the config's model.tracer, else numpy)")
    ap.add_argument('--factors', choices=['numpy', 'hip'],
                    help="where the Doppler factor and the transport factors J are computed (default: the config's model.factors, else numpy)")
    ap.add_argument('--resident', action='store_true',
                    help="keep the geodesic record, Omega, g, J and the ray-tracing arguments on the GPU (needs --tracer hip --factors hip)")
    args = ap.parse_args()
    with open(args.config) as f:
        config = yaml.safe_load(f)
    pre, model, opt_cfg = config['preprocess'], config['model'], config['optimization']
    if args.tracer:
        model['tracer'] = args.tracer
    if args.factors:
        model['factors'] = args.factors
    if not os.path.exists(pre['data_path']):
        synthetic_flare(pre['data_path'], dict(model, resident=False), pre)          # (rendered on the host from NumPy arguments)
    if args.resident:
        model['resident'] = True

    # data: window-averaged light curves, split in time into a training and a validation part
    target, t_frames = bhnerf.alma.preprocess_data(**pre)
    split = pre['t_start'] * units.hr + opt_cfg['train_split'] * units.min
    train, val = np.asarray(t_frames <= split), np.asarray(t_frames > split)
    sigma = np.asarray(opt_cfg['sigma'], dtype=np.float64)
    train_step = bhnerf.optimization.TrainStep.image(t_frames[train], target[train], sigma, dtype='lc')
    val_step = bhnerf.optimization.TrainStep.image(t_frames[val], target[val], sigma, dtype='lc')

    rmax = model['fov_M'] / 2.0
    rmin = float(bhnerf.constants.isco_pro(model['spin'])) if model['rmin'] == 'ISCO' else model['rmin']
    predictor = bhnerf.network.NeRF_Predictor(rmax, rmin, rmax, model['z_width'])
    rot_angle = np.deg2rad(pre['de_rot_angle'] + 20.0)
    hparams = dict(opt_cfg['hparams'])
    seeds = args.seeds or [hparams['seed']]
    runname = 'inc_{:.1f}.seed_{}'
    stokes = ['I', 'Q', 'U']

    for inc in args.inc:
        rt_args = bhnerf.alma.get_raytracing_args(np.deg2rad(inc), model['spin'], model, rot_angle=rot_angle)
        for seed in seeds:
            ckpt = os.path.join(opt_cfg['checkpoint_dir'], runname.format(inc, seed))
            if os.path.exists(ckpt):
                continue                                                            # finished earlier
            writer = bhnerf.optimization.SummaryWriter(logdir=os.path.join(opt_cfg['log_dir'], runname.format(inc, seed)))
            period = opt_cfg['log_period']
            log_fns = [
                LogFn(lambda o: writer.add_scalar('log_loss/train', np.log10(np.mean(o.loss)), global_step=o.step)),
                LogFn(lambda o: writer.recovery_3d(model['fov_M'], vis_res=32)(o), log_period=period),
                LogFn(lambda o: writer.plot_lc_datafit(o, 'training', train_step, target[train], stokes, t_frames[train]), log_period=period),
                LogFn(lambda o: writer.plot_lc_datafit(o, 'validation', val_step, target[val], stokes, t_frames[val]), log_period=period),
            ]
            hparams['seed'] = seed
            optimizer = bhnerf.optimization.Optimizer(hparams, predictor, rt_args, save_period=hparams['num_iters'], checkpoint_dir=ckpt)
            optimizer.run(opt_cfg['batchsize'], train_step, rt_args, log_fns=log_fns)
            writer.close()
            fit = bhnerf.optimization.total_movie_loss(opt_cfg['batchsize'], optimizer.state, train_step, rt_args)
            held = bhnerf.optimization.total_movie_loss(opt_cfg['batchsize'], optimizer.state, val_step, rt_args)
            print('inc %5.1f seed %d: chi2/frame train %.3f  validation %.3f' % (inc, seed, fit, held))

    fmt = os.path.join(opt_cfg['checkpoint_dir'], 'inc_{:.1f}.seed_{}')
    table = bhnerf.alma.chi2_df(args.inc, model['spin'], seeds, model, fmt, t_frames[train], target[train], stokes, sigma=sigma,
                                rot_angle=rot_angle, final_step=hparams['num_iters'])
    print(table)


if __name__ == '__main__':
    main()
