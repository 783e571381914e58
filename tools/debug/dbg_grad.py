import os, sys, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from gpu_support import chi2_step, predictor_of, ray_args
from mlp_problems import oracle_trainer, random_problem_inputs
from conftest import golden_tree
dev = torch.device('cuda:0')
def run(width, depth, S, H=9, Wd=7, G=50, B=3):
    prob = random_problem_inputs(width, depth, S, 3, shape=(H, Wd, G, B))
    g, t_frames, t_inj, target, sigma, offset = (prob[k] for k in ('g', 't_frames', 't_inj', 'target', 'sigma', 'offset'))
    tr, t = oracle_trainer(g)
    loss_ref, img_ref, grads_ref = tr.loss_and_grad(t(t_frames), t(target), t(sigma), t(offset), 1.0, 'full')
    n = len(tr.k)
    pred, rt = predictor_of(g, 'bf16', dev), ray_args(g)
    eng = pred.engine()
    gd = chi2_step(pred, eng.flatten(golden_tree(g)), rt, t_frames, target, sigma, offset)[2]
    gmax = max(float(x.abs().max()) for x in grads_ref)
    for i in range(n):
        k = gd[eng.kernel_off[i]:eng.kernel_off[i] + eng.in_dim[i] * eng.out_dim[i]].reshape(eng.in_dim[i], eng.out_dim[i])
        b = gd[eng.bias_off[i]:eng.bias_off[i] + eng.out_dim[i]]
        ek = np.abs(k - grads_ref[i].numpy()); eb = np.abs(b - grads_ref[n + i].numpy())
        w = np.unravel_index(ek.argmax(), ek.shape)
        print('W%d D%d S%d layer %d: kernel err %.2e (at %s, ref %.3e dev %.3e) bias err %.2e | rows-err max by in-block: %s' % (
            width, depth, S, i, ek.max() / gmax, w, grads_ref[i].numpy()[w], k[w], eb.max() / gmax,
            ['%.1e' % (ek[j:j + 32].max() / gmax) for j in range(0, ek.shape[0], 32)]))
import sys as _s
MODE = 'bf16'
run(128, 4, 3); run(256, 4, 0)
