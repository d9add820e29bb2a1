"""`train.Captured` on the device: the warm-up runs for real and the captures execute nothing, each callable is a
graph of its own that replays what it did, and a replay refuses an optimizer whose state was loaded after the capture."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_two_callables_on_one_counter():
    from mrgcn_amd.train import Captured
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")

    def f0():
        return ctr.add_(1)

    def f1():
        return ctr.add_(10)

    def warmup():
        f0()
        f1()
        assert int(ctr) == 11   # (the warm-up is real)
        ctr.zero_()
    cap = Captured([f0, f1], warmup)
    assert int(ctr) == 0 and len(cap.graphs) == 2 and cap.pair_sums == [[], []]
    outs = [cap.replay(0), cap.replay(0), cap.replay(1), cap.replay(), cap.replay(1)]
    assert int(ctr) == 23
    assert all(o is cap.outs[0] for o in (outs[0], outs[1], outs[3])) and outs[2] is cap.outs[1] is outs[4]
    assert cap.outs[0] is ctr and cap.outs[1] is ctr


def test_a_replay_refuses_an_optimizer_state_loaded_after_the_capture():
    from mrgcn_amd._lib import MrgcnError
    from mrgcn_amd.train import Captured, ClipAdam
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(4, 4, device="cuda"))
    opt = ClipAdam([p], lr=0.01, max_norm=1.0, capturable=True)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = (p * p).sum()
        loss.backward()
        opt.step()
        return loss.detach()
    guarded = Captured([step], step, opt, who="a test's step")
    free = Captured([step], step)
    first = float(guarded.replay())
    assert float(guarded.replay()) < first   # (the replays step the parameter)
    kept = (dict(opt.state), dict(opt._dev_step))   # (the buffers the graphs name stay allocated for the last replay)
    opt.load_state_dict(opt.state_dict())
    with pytest.raises(MrgcnError, match="a test's step: the optimizer's state was loaded after the capture"):
        guarded.replay()
    free.replay()   # (no optimizer given: nothing to compare)
    torch.cuda.synchronize()
    del kept
