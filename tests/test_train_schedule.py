"""CPU: host logic of the captured training step - the filter-gradient schedule context and the no-trace guard."""
import pytest
import torch

from faster_rcnn_pytorch_multimodal_amd.model import train_graph
from faster_rcnn_pytorch_multimodal_amd.nets import autograd_ops as A


def test_wgrad_schedule_context_installs_and_restores():
    assert A.SCHEDULE is A.EAGER_SCHEDULE
    assert A.EAGER_SCHEDULE == A.WgradSchedule(accumulate=False, side_stream=False, grouped=False, bn_stat_sink=None)
    with pytest.raises(AttributeError):
        A.EAGER_SCHEDULE.grouped = True                       # a record, not a bag of switches
    forked = A.WgradSchedule(accumulate=True, side_stream=True, grouped=True, bn_stat_sink=None)
    chain = A.WgradSchedule(accumulate=True, side_stream=False, grouped=True, bn_stat_sink={})
    with A.wgrad_schedule(forked) as installed:
        assert installed is forked and A.SCHEDULE is forked
        with A.wgrad_schedule(chain):
            assert A.SCHEDULE is chain
            with pytest.raises(ValueError, match="stop"):
                with A.wgrad_schedule(A.EAGER_SCHEDULE):
                    assert A.SCHEDULE is A.EAGER_SCHEDULE
                    raise ValueError("stop")
            assert A.SCHEDULE is chain                        # back after a body that raised
        assert A.SCHEDULE is forked                           # nesting restores in order
    assert A.SCHEDULE is A.EAGER_SCHEDULE


@pytest.mark.parametrize("raises", [True, False])
def test_leaves_no_trace_restores_gradients_statistics_and_draw_counter(raises):
    torch.manual_seed(4)
    net = torch.nn.Sequential(torch.nn.Conv2d(4, 4, 1), torch.nn.BatchNorm2d(4))
    net.train()
    bn = net[1]
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(4))
        bn.running_var.copy_(torch.rand(4) + 0.5)
        bn.num_batches_tracked.fill_(7)
    for p in net.parameters():
        p.grad = torch.randn_like(p)
    net._uc_calls = 5
    grads = [p.grad for p in net.parameters()]
    before = [g.clone() for g in grads] + [bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()]

    def body():
        with train_graph.leaves_no_trace(net, grads, [bn]):
            for g in grads:
                g.fill_(3.0)
            net(torch.randn(2, 4, 5, 5) * 4 + 1)
            assert int(bn.num_batches_tracked) == 8 and not torch.equal(bn.running_mean, before[-3])
            net._uc_calls = 9
            if raises:
                raise ValueError("stop")

    if raises:
        with pytest.raises(ValueError, match="stop"):
            body()
    else:
        body()
    after = [p.grad for p in net.parameters()] + [bn.running_mean, bn.running_var, bn.num_batches_tracked]
    assert all(a is g for a, g in zip(after, grads))          # the same buffers ...
    assert all(torch.equal(a, b) for a, b in zip(after, before))          # ... holding the same bits
    assert net._uc_calls == 5
