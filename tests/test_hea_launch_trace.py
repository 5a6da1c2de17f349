"""What the MFMA engine's host launches (no GPU needed): for every case of tools/hea_launch_trace.py the launches of
each scripted call - names, flags, geometry lists, workspace buffers by name, pass tables by identity - and the
program's tables and per-plan constants equal tests/golden/hea_launch_traces.json, recorded before the host was
restructured around ``HeaMfmaProgram._launch``.  A second test reads the routes of a training step straight from the
traces."""
import importlib.util
import json
import os

import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_sp = importlib.util.spec_from_file_location("hea_launch_trace", os.path.join(_ROOT, "tools", "hea_launch_trace.py"))
lt = importlib.util.module_from_spec(_sp)
_sp.loader.exec_module(lt)

with open(lt.GOLDEN) as _f:
    GOLDEN = json.load(_f)

_TRACES = {}


def _trace(name):
    """The record-mode trace of a case, as JSON data (traced once per process)."""
    if name not in _TRACES:
        _TRACES[name] = json.loads(json.dumps(lt.trace_case(name)[0]))
    return _TRACES[name]


def test_golden_covers_the_cases():
    assert sorted(GOLDEN) == sorted(lt.CASES)
    assert os.path.getsize(lt.GOLDEN) < 200 * 1024
    for name, case in lt.CASES.items():
        assert sorted(GOLDEN[name]["calls"]) == sorted(case["script"])


@pytest.mark.parametrize("name", sorted(lt.CASES))
def test_trace_equals_golden(name):
    got, want = _trace(name), GOLDEN[name]
    for what in lt.CASES[name]["script"]:
        g, w = got["calls"][what], want["calls"][what]
        if g != w:
            i = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            print(f"{name} / {what}: {len(g)} launches, golden {len(w)}; first difference at launch {i}")
            print("  got   ", json.dumps(g[i]) if i < len(g) else None)
            print("  golden", json.dumps(w[i]) if i < len(w) else None)
        assert g == w, f"{name}: launches of {what}"
    assert got["header"] == want["header"]
    assert got["counters"] == want["counters"] and got["refused"] == want["refused"]


def _passes(calls):
    return [c for c in calls if c[0] == "hea_pass"]


def _readout_list(c):
    """The fused readout's tensor list of a ``hea_pass`` launch (positional argument 17), or None."""
    return c[2][17] if len(c[2]) > 17 else None


@pytest.mark.parametrize("name", sorted(lt.CASES))
def test_routes_of_a_step(name):
    tr = _trace(name)
    J, R = tr["header"]["n_passes"], tr["header"]["fwd_last"]
    for what, calls in tr["calls"].items():
        if not (what.startswith("step") or what.startswith("dpsgd")):
            continue
        # every step: forward passes 0..fwd_last, then adjoint passes J-1..0
        assert [c[1] for c in _passes(calls)] == [f"fwd{j}" for j in range(R + 1)] + \
            [f"adj{j}" for j in range(J - 1, -1, -1)], (name, what)
    step = tr["calls"]["step"]
    names = [c[0] for c in step]
    mode = tr["header"]["readout_mode_S"]
    adj = [c for c in _passes(step) if c[1].startswith("adj")]
    first_adj = step.index(adj[0])
    if mode == "fused":
        with_ro = [c for c in _passes(step) if _readout_list(c) is not None]
        assert with_ro == [adj[0]] and adj[0][1] == f"adj{J - 1}" and adj[0][3]["spec"] is False
        assert "hea_readout_rec" not in names and "readout_ce" not in names
    elif mode == "split":
        assert names.count("hea_readout_rec") == 1 and names[first_adj - 1] == "hea_readout_rec"
        assert all(c[3]["spec"] is True and _readout_list(c) is None for c in adj)
    else:
        assert mode == "kernel" and names.count("readout_ce") == 1
        assert names[first_adj - 1] == "readout_ce" and step[first_adj - 2][1] == f"fwd{R}"
        assert all(_readout_list(c) is None for c in adj)


def test_the_cases_reach_every_route():
    modes = {name: GOLDEN[name]["header"]["readout_mode_S"] for name in GOLDEN}
    assert modes["10q2L_t8_s160"] == "split" and modes["10q2L_t8_split_on"] == "split"
    assert modes["10q2L_t8_split_off"] == "fused" and modes["10q2L_t8"] == "fused" and modes["12q3L_t8_c8"] == "kernel"
    assert GOLDEN["10q1L_t8"]["header"]["fwd_last"] == 0 and GOLDEN["10q1L_t8"]["header"]["n_passes"] == 2
    assert GOLDEN["12q1L_t8"]["header"]["fwd_last"] == 0 and GOLDEN["12q1L_t8"]["header"]["n_passes"] == 3
    assert GOLDEN["12q4L_t9"]["header"]["n_passes"] == 4
    assert GOLDEN["10q2L_t8_interp"]["counters"]["step"][0] == 0 and GOLDEN["10q2L_t8_gen"]["counters"]["step"][1] == 1
