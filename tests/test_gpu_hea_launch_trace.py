"""The CPU launch traces (tests/golden/hea_launch_traces.json, tests/test_hea_launch_trace.py) are what the device
runs: with the recorder of tools/hea_launch_trace.py forwarding every call, a real training step, ``expz`` and ``vjp``
issue exactly the golden launch lists of the same cases, and their results are finite and equal, bit for bit, those
of a second program that ran without the recorder."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_sp = importlib.util.spec_from_file_location("hea_launch_trace", os.path.join(_ROOT, "tools", "hea_launch_trace.py"))
lt = importlib.util.module_from_spec(_sp)
_sp.loader.exec_module(lt)

SCRIPT = ("step", "expz", "vjp")


@pytest.mark.parametrize("name", ["10q2L_t8_gen", "16q3L_interp"])
def test_device_runs_the_recorded_launches(name, tmp_path):
    with open(lt.GOLDEN) as f:
        golden = json.load(f)[name]
    dev = torch.device("cuda", 0)
    trace, res, prog = lt.trace_case(name, dev, passthrough=True, script=SCRIPT, jit_cache=tmp_path)
    torch.cuda.synchronize()
    trace = json.loads(json.dumps(trace))
    for what in SCRIPT:
        assert trace["calls"][what] == golden["calls"][what], what
    assert trace["header"] == golden["header"]
    assert prog.spec_active == lt.CASES[name]["prog"]["use_spec"]
    with lt.case_env(name, tmp_path):
        plain = lt.build_program(name, dev)
        inp = lt.case_inputs(name, dev)
        for what in SCRIPT:
            want = lt.tensors(lt.clone(lt.run_call(plain, name, what, inp)))
            torch.cuda.synchronize()
            got = lt.tensors(res[what])
            assert len(got) == len(want) > 0
            for a, b in zip(got, want):
                assert torch.isfinite(a).all(), what
                assert a.dtype == b.dtype and torch.equal(a, b), what
