import sys, os, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from conftest import golden_tree
from gpu_support import chi2_step, predictor_of, ray_args
from mlp_bounds import l2err, relerr
from mlp_problems import flat_grad, oracle_trainer, targets
from bhnerf_amd import network, units
dev = torch.device('cuda:0')
G = lambda n: dict(np.load(os.path.join(ROOT, 'tests', 'golden', '%s.npz' % n)))
for tag in 'abcdef':
    g = G('g5_predict_' + tag)
    for mode in ('f32', 'bf16'):
        # forward
        pred, tree = predictor_of(g, mode, dev), golden_tree(g)
        e = pred.apply({'params': tree}, g['t_frames'], units.hr, g['coords'].astype(np.float32), g['Omega'].astype(np.float32),
                       float(g['t_start_obs']), g['t_geos'].astype(np.float32), float(g['t_injection'])).cpu().numpy()
        mism = ((e == 0) != (g['emission'] == 0))
        same = ~mism
        f = lambda k: g[k].astype(np.float32)
        J = f('J') if g['J'].ndim else 1.0
        with torch.no_grad():
            images = network.image_plane_prediction(tree, pred.apply, g['t_frames'], f('coords'), f('Omega'), J, f('g'), f('dtau'), f('Sigma'), float(g['t_start_obs']), f('t_geos'), float(g['t_injection']), units.hr).cpu().numpy()
        line = '%s %-4s W=%d mism %d/%d  e_err %.2e  img_err %.2e' % (tag, mode, int(g['hparams'][6]), mism.sum(), mism.size, relerr(e[same], g['emission'][same]), relerr(images, g['images']))
        for dt in ('full', 'lc'):
            tr, t = oracle_trainer(g)
            tg = targets(g, dt)
            scale = float(g['hparams'][7])
            loss_ref, _, grads_ref = tr.loss_and_grad(t(g['t_frames']), t(tg['target']), t(tg['sigma']), t(tg['offset']), scale, dt)
            gref = flat_grad(grads_ref)
            pred2, rt = predictor_of(g, mode, dev), ray_args(g)
            loss, _, gdev = chi2_step(pred2, pred2.engine().flatten(golden_tree(g)), rt, g['t_frames'], tg['target'], tg['sigma'], tg['offset'], scale, dt)
            gdev = gdev.astype(np.float64)
            line += '  | %s: L2 %.2e max %.2e loss %.1e' % (dt, l2err(gdev, gref), np.abs(gdev - gref).max() / np.abs(gref).max(), abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()))
        print(line, flush=True)
