"""What tests/test_madgrad_adais_host.py and tests/test_madgrad_adais_gpu.py share: the fixture recorded from the reference's own MADGRAD and
AdaiS (tests/golden/optim_ref_trajectories.npz, written by tests/golden/make_optim_golden.py on the CPU)."""
import os

import torch

from optim_harness import TrajectoryFixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_ref_trajectories.npz")
CASES = ["madgrad_recipe", "madgrad_alt", "adais_recipe", "adais_alt"]


class Fixture(TrajectoryFixture):
    """the file stores the gradients; AdaiS cases add the mean of the bias-corrected second moment per step, float64 and float32"""

    GOLDEN = GOLDEN

    def __init__(self, case):
        super().__init__(case)
        self.grads = torch.from_numpy(self.rec("grads"))
        if self.cls == "AdaiS":
            self.mean64, self.mean32 = self.rec("mean64"), self.rec("mean32")
