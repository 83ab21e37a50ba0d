"""Golden fixture for the learning-rate schedule: the float64 rates the REFERENCE's own scheduler (train_utils/lr_schedulers.py,
get_scheduler('cosine', ...), imported unmodified) writes into `param_group['lr']`, recorded by `scheduler.step(k); get_last_lr()`.
Recorded numbers only - no reference source is copied.  Yardstick of tests/test_lr_schedule_cpu.py (bit equality) and of the index
grid of tests/test_hip_optim_device_step.py.  Build container only:
    python tests/golden/make_golden_lr.py"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

LONG = [0, 1, 2, 999, 1000, 1001, 300500, 599999, 600000, 600001, 900000, 1200000]
# name -> (base_lr, end_lr, warmup_steps, training_steps, indices): the reference's generator and discriminator (configs/tiny.yaml: lr
# 1e-4, disc_lr_ratio 0.15, end_lr a tenth), no warm-up, and a warm-up as long as the run
SETS = {
    "gen": (1e-4, 1e-5, 1000, 600000, LONG),
    "disc": (1.5e-5, 1.5e-6, 1000, 600000, LONG),
    "nowarm": (1e-4, 0.0, 0, 10, list(range(25))),
    "allwarm": (3e-4, 1e-5, 5, 5, list(range(25))),
}


def main():
    from train_utils.lr_schedulers import get_scheduler
    out = {}
    for name, (base_lr, end_lr, warmup, total, indices) in SETS.items():
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=base_lr)
        sched = get_scheduler("cosine", opt, num_warmup_steps=warmup, num_training_steps=total, base_lr=base_lr, end_lr=end_lr)
        rates = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # the epoch argument of step() is deprecated, not removed
            for k in indices:
                sched.step(k)
                (lr,) = sched.get_last_lr()
                assert lr == opt.param_groups[0]["lr"]
                rates.append(lr)
        out[name + "_params"] = np.array([base_lr, end_lr, warmup, total], dtype=np.float64)
        out[name + "_indices"] = np.array(indices, dtype=np.int64)
        out[name + "_rates"] = np.array(rates, dtype=np.float64)
        print(name, rates[:3], "...", rates[-1])
    np.savez(os.path.join(HERE, "lr_schedule_kat.npz"), **out)
    print("wrote lr_schedule_kat.npz", os.path.getsize(os.path.join(HERE, "lr_schedule_kat.npz")), "bytes")


if __name__ == "__main__":
    main()
