"""The order of one pass through a step's graph chain (fastvim_amd/graph_chain.py: ``run_chain``), driven with recording
fakes: no device, milliseconds."""
import pytest

from fastvim_amd.graph_chain import capture_mode, run_chain


class _Graph:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def replay(self):
        self.log.append(self.name)


class _Exchange:
    def __init__(self, log):
        self.log = log

    def launch(self, k):
        self.log.append(f"L{k}")

    def finish(self, mean=True):
        self.log.append(f"finish(mean={mean})")


def _chain(K):
    log = []
    return log, _Graph(log, "fwd"), [_Graph(log, f"b{k}") for k in range(K)], _Graph(log, "opt"), _Exchange(log)


def _run(fwd, bwd, opt, ex, **kw):
    return run_chain(fwd.replay, [g.replay for g in bwd], opt.replay, ex, **kw)


@pytest.mark.parametrize("K", [1, 3])
def test_exchanged_pass_launches_each_bucket_behind_its_backward_graph(K):
    log, fwd, bwd, opt, ex = _chain(K)
    _run(fwd, bwd, opt, ex, exchange=True)
    assert log == ["fwd"] + [s for k in range(K) for s in (f"b{k}", f"L{k}")] + ["finish(mean=False)", "opt"]
    if K == 3:
        assert log == ["fwd", "b0", "L0", "b1", "L1", "b2", "L2", "finish(mean=False)", "opt"]


def test_exchange_is_the_default_and_the_forward_result_is_returned():
    log, fwd, bwd, opt, ex = _chain(1)
    assert run_chain(lambda: (fwd.replay(), "loss")[1], [bwd[0].replay], opt.replay, ex) == "loss"
    assert log == ["fwd", "b0", "L0", "finish(mean=False)", "opt"]


def test_a_micro_batch_that_is_not_the_last_stops_after_backward():
    log, fwd, bwd, opt, ex = _chain(3)
    _run(fwd, bwd, opt, ex, exchange=False)
    assert log == ["fwd", "b0", "b1", "b2"]


def test_launch_and_finish_replaced_on_the_instance_are_the_ones_called():
    log, fwd, bwd, opt, ex = _chain(3)
    launch, finish = ex.launch, ex.finish
    ex.launch = lambda k: (log.append(f"mine{k}"), launch(k))[1]
    ex.finish = lambda mean=True: (log.append("mine"), finish(mean=mean))[1]
    _run(fwd, bwd, opt, ex)
    assert log == ["fwd", "b0", "mine0", "L0", "b1", "mine1", "L1", "b2", "mine2", "L2", "mine", "finish(mean=False)", "opt"]


def test_time_exposed_brackets_finish_alone():
    import contextlib
    log, fwd, bwd, opt, ex = _chain(2)

    @contextlib.contextmanager
    def bracket():
        log.append("e0")
        yield
        log.append("e1")

    _run(fwd, bwd, opt, ex, time_exposed=bracket)
    assert log == ["fwd", "b0", "L0", "b1", "L1", "e0", "finish(mean=False)", "e1", "opt"]
    del log[:]
    _run(fwd, bwd, opt, ex, exchange=False, time_exposed=bracket)       # nothing to wait for: no bracket either
    assert log == ["fwd", "b0", "b1"]


def test_capture_mode_without_a_process_group_is_global():
    assert capture_mode() == "global"
