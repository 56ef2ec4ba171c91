#!/usr/bin/env python3
"""The headline bench batch, a few infer calls (for rocprofv3 --kernel-trace --stats)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from gpu_util import make_net
from mb_istft_vits_amd import synth
net, _ = make_net("ljs_mb_istft_vits")
x, xl, _ = synth.synthetic_batch(net.cfg, 64, 200, seed=0, ragged="--ragged" in sys.argv)
x, xl = torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda()
for _ in range(8):
    net.infer(x, xl, noise_scale=0, length_scale=1)
torch.cuda.synchronize()
