"""Generate tests/golden/mobilenet_v1.npz by IMPORTING the reference's lib/nets/mobilenet_v1.py (read-only,
/root/reference).  Run only in the build container, once (the reference never travels to the GPU box):

    python -B tests/golden/make_golden_mobilenet.py

``nets.network`` is missing from the reference snapshot, so a stub module with an empty ``Network`` class is registered
before the import, and the easydict stand-in of make_golden.py before ``model.config``.  ``mobilenet_v1_base()`` is
filled with ``tests/mobilenet_restatement.seeded_state`` (weights from names, shapes and a seed) and evaluated in fp32.

Stored (data only, no weights, no program text): the ordered key / shape list of the body's state dict, a float64
checksum per seeded tensor, the input (1,3,50,84) (odd and even maps meet the three stride-2 depthwise layers), the head
output (1,512,4,6), a pooled input (2,512,7,7) in U(0,6) and ``tail(pooled).mean(3).mean(2)`` (2,1024).

Checked while generating (float64 restatement): every one of the 14 stages keeps a healthy share of its values strictly
inside (0,6) and some at 6 - no layer dies or saturates - and the fp32-vs-float64 gap of both outputs is printed.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF_LIB = "/root/reference/lib"

sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_golden import _install_easydict_stand_in      # noqa: E402
import mobilenet_restatement as R                        # noqa: E402


def main():
    _install_easydict_stand_in()
    sys.path.insert(0, REF_LIB)
    stub = types.ModuleType("nets.network")
    stub.Network = type("Network", (torch.nn.Module,), {})
    import nets                                                     # reference package
    sys.modules["nets.network"] = stub
    nets.network = stub
    import nets.mobilenet_v1 as ref                                 # reference

    torch.manual_seed(0)
    body = ref.mobilenet_v1_base().eval()
    sd = body.state_dict()
    shapes = [(k, tuple(v.shape)) for k, v in sd.items()]
    assert shapes == R.key_shapes(), "the restatement's key / shape table differs from the reference's"
    state = R.seeded_state(shapes)
    body.load_state_dict(R.torch_state(state, torch.float32))
    head = torch.nn.Sequential(*list(body.children())[:12])
    tail = torch.nn.Sequential(*list(body.children())[12:])

    rng = np.random.default_rng(R.SEED + 1)
    x = rng.normal(0.0, 1.0, (1, 3, 50, 84)).astype(np.float32)
    pooled = rng.uniform(0.0, 6.0, (2, 512, 7, 7)).astype(np.float32)
    with torch.no_grad():
        head_out = head(torch.from_numpy(x).clone()).numpy()
        tail_out = tail(torch.from_numpy(pooled).clone()).mean(3).mean(2).numpy()
    assert head_out.shape == (1, 512, 4, 6) and tail_out.shape == (2, 1024)

    s64 = R.torch_state(state, torch.float64)
    stages = []
    h64 = R.head(s64, torch.from_numpy(x).double(), stages).numpy()
    t64 = R.tail(s64, torch.from_numpy(pooled).double(), stages).numpy()
    for i, s in enumerate(stages):
        inside = float(((s > 0) & (s < 6)).double().mean())
        at6 = float((s == 6).double().mean())
        print("stage %2d  %-18s inside (0,6) %5.1f %%   at 6 %5.2f %%" % (i, tuple(s.shape), 100 * inside, 100 * at6))
        assert inside >= 0.25, "stage %d is dead or saturated" % i
    print("reference fp32 vs float64 restatement: net_conv %.3g, fc7 %.3g"
          % (np.abs(head_out - h64).max(), np.abs(tail_out - t64).max()))

    sums = R.checksums(state)
    out = os.path.join(HERE, "mobilenet_v1.npz")
    np.savez_compressed(out, keys=np.array([k for k, _ in shapes]),
                        shapes=np.array([",".join(str(d) for d in s) for _, s in shapes]),
                        checksums=np.array([sums[k] for k, _ in shapes], dtype=np.float64),
                        seed=np.int64(R.SEED), x=x, head_out=head_out, pooled=pooled, tail_out=tail_out)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
