"""Generate tests/golden/basicblock.npz by IMPORTING the reference's lib/nets/resnet.py (read-only, /root/reference) and running
its own ``BasicBlock`` class (resnet.py:34-71).  Run only in the build container, once (the reference never travels to the GPU
box):

    python -B tests/golden/make_golden_basicblock.py

``resnet18()`` / ``resnet34()`` raise TypeError in the reference (``_make_layer`` hands BasicBlock keywords it does not take), so
the whole nets cannot be run there; the block's class constructs on its own.  Two blocks on an 8-channel 6 x 5 map (odd width,
two images), each filled with ``tests/resnet_basic_restatement.seeded_from_shapes`` (weights from names, shapes and a seed) and
evaluated in eval mode in fp32:

    plain   BasicBlock(8, 8)                        stride 1, no shortcut             -> (2, 8, 6, 5)
    down    BasicBlock(8, 16, stride=2, downsample=Sequential(conv1x1(8, 16, 2), BatchNorm2d(16)))  -> (2, 16, 3, 3)

Stored (data only, no weights, no program text): the seeds, the input, both outputs, and the ordered key list of each block's
state dict.  Checked while generating: the restatement's key / shape tables equal the reference's, and the float64 restatement
agrees with the reference's fp32 outputs to fp32 rounding.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF_LIB = "/root/reference/lib"

sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_golden import _install_easydict_stand_in      # noqa: E402
import resnet_basic_restatement as R                     # noqa: E402


def main():
    _install_easydict_stand_in()
    sys.path.insert(0, REF_LIB)
    import nets.resnet as ref                                       # reference

    rng = np.random.default_rng(R.SEED + 2)
    x = rng.standard_normal((2, 8, 6, 5)).astype(np.float32)
    saved = {"x": x, "seed_plain": np.int64(R.SEED + 3), "seed_down": np.int64(R.SEED + 4)}
    for name, inplanes, planes, stride in (("plain", 8, 8, 1), ("down", 8, 16, 2)):
        down = None
        if name == "down":
            down = torch.nn.Sequential(ref.conv1x1(inplanes, planes, stride), torch.nn.BatchNorm2d(planes))
        blk = ref.BasicBlock(inplanes, planes, stride, down).eval()
        shapes = [(k, tuple(v.shape)) for k, v in blk.state_dict().items()]
        assert shapes == R.block_shapes("", inplanes, planes, down is not None), "the restatement's key / shape table differs"
        state = R.seeded_from_shapes(shapes, int(saved["seed_" + name]))
        blk.load_state_dict(state, strict=True)
        with torch.no_grad():
            y = blk(torch.from_numpy(x).clone()).numpy()
            y64 = R.block(state, "", torch.from_numpy(x).double(), stride).numpy()
        gap = float(np.abs(y - y64).max())
        print("%s: output %s, positive %.2f, reference fp32 vs float64 restatement %.3g" % (name, y.shape, float((y > 0).mean()), gap))
        assert gap < 1e-5 and float((y > 0).mean()) > 0.25
        saved["y_" + name] = y
        saved["keys_" + name] = np.array([k for k, _ in shapes])
    out = os.path.join(HERE, "basicblock.npz")
    np.savez_compressed(out, **saved)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
