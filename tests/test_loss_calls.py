"""ChainLoss makes the recorded library calls: one training step - forward, backward over a retained graph, backward again - of
every combination of xent regularisation, the output regularisers, utterance / derivative weights and averaging, on CPU tensors
and (gpu) on the three device routes with the lengths on either side, under a proxy that writes down every pychain_hip_* call
with its scalar arguments and which pointers are null (tests/golden/make_loss_calls.py).  What is compared is the recorded
sequence of entry-point families and a hash of the full trace; a mismatch prints the full trace, and
`python tests/golden/make_loss_calls.py --dump CONFIG` prints it at any other commit for a diff.  A change of what a step
launches regenerates the file on purpose; a refactor does not."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_loss_calls", os.path.join(GOLDEN, "make_loss_calls.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
with open(os.path.join(GOLDEN, "loss_calls.json")) as _f:
    RECORDED = json.load(_f)


def _check(section, name):
    seq, digest = RECORDED[section]["configs"][name]
    want = RECORDED[section]["sequences"][seq]
    trace = gen.step(name)
    names, got = gen.summary(trace)
    if (names, got) != (want, digest):
        print("recorded: %s\ngot:      %s\n%s" % (want, names, json.dumps(trace, indent=1, sort_keys=True)))
    assert names == want
    assert got == digest, "the same entry points, other arguments: see the trace printed above"


def test_the_recorded_configurations_are_the_grid():
    assert list(RECORDED["cpu"]["configs"]) == gen.configs("cpu") and len(gen.configs("cpu")) == 32
    assert list(RECORDED["gpu"]["configs"]) == gen.configs("gpu") and len(gen.configs("gpu")) == 192 + 3 * 16 + 8


@pytest.mark.parametrize("name", gen.configs("cpu"))
def test_cpu_step_makes_the_recorded_calls(name):
    _check("cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", gen.configs("gpu"))
def test_gpu_step_makes_the_recorded_calls(name):
    _check("gpu", name)
