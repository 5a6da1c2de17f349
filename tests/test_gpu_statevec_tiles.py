"""The generic statevector kernels at every tile shape against float64.

Every case of tests/statevec_cases.py runs on the interpreter kernel (csrc/statevec.hip) and the listed ones also on
the per-plan kernels (csrc/jit.cpp), with ``HipProgram(kmax=)`` forcing tiles of 1..256 threads and qubits outside the
tile.  The reference is the torch executor in complex128 on the CPU from the same float32 inputs; tests/
test_statevec_tiles.py proves on the CPU which kernel branches each case reaches.  Bounds: the engine's existing ones
(tests/test_gpu_simulator.py) applied against float64 - 2e-5 on amplitudes and <Z>, 5e-5 on gradients.  The measured
errors are recorded next to the fp32 torch executor's own in profiles/statevec_tiles_err_table.txt
(tools/statevec_tiles_err_table.py)."""
import functools

import pytest
import torch

from qfedx_amd.ops.statevec_hip import HipProgram
from tests import statevec_cases as sc

pytestmark = pytest.mark.gpu

TOL = dict(psi=2e-5, z=2e-5, z_eval=2e-5, z_vjp=2e-5, grad=5e-5)
S, K, B = sc.S_SAMPLES, sc.K_ROWS, sc.B_SAMPLES
_BF16_NAN = 0x7FC07FC0             # two bf16 NaNs


def make_program(case, device, jit: bool, state_dtype: str = "fp32") -> HipProgram:
    ops, coef = case.program()
    prog = HipProgram(ops, coef, case.n, list(case.readout), device, case.n_theta, state_dtype=state_dtype,
                      kmax=case.kmax, jit=jit, x_width=case.x_width)
    assert prog.R == case.R and prog.train_plan.k == case.kmax
    return prog


def pad_workspaces(prog: HipProgram) -> dict:
    """psi / lam / part / slab sized for S + 1 samples and filled with NaN; returns name -> used element count.
    The kernels must write every entry of the S samples they read later and nothing past them."""
    tps = prog.train_plan.tiles_per_state
    used = dict(psi=S << prog.n, lam=S << prog.n, part=S * tps * prog.C, slab=S * tps * prog.G)
    for name, cnt in used.items():
        numel = cnt // S * (S + 1)
        if name in ("psi", "lam"):
            if prog.bf16:
                t = torch.full((numel,), _BF16_NAN, dtype=torch.int32, device=prog.device)
            else:
                t = torch.full((numel,), complex(float("nan"), float("nan")), dtype=torch.complex64,
                               device=prog.device)
        else:
            t = torch.full((numel,), float("nan"), dtype=torch.float32, device=prog.device)
        prog._ws[name] = t
    return used


def assert_padding_untouched(prog: HipProgram, used: dict) -> None:
    for name, cnt in used.items():
        t = prog._ws[name]
        assert t.numel() == cnt // S * (S + 1), f"{name} workspace was reallocated"
        tail = t[cnt:]
        if t.dtype == torch.int32:
            assert bool((tail == _BF16_NAN).all()), f"{name}: write past sample S - 1"
        else:
            assert bool(torch.view_as_real(tail).isnan().all() if t.is_complex() else tail.isnan().all()), \
                f"{name}: write past sample S - 1"


def _once(prog: HipProgram, name: str) -> dict:
    inp = sc.inputs(name)
    dev = prog.device
    x, th, w = inp["x"].to(dev), inp["theta"].to(dev), inp["w"].to(dev)
    out = {}
    for start, init in (("prod", None), ("cplx", inp["init_c"].to(dev)), ("real", inp["init_r"].to(dev))):
        psi, z = prog.statevector(x, th, init)
        z_vjp, grad = prog.vjp(x, th, w, init)
        out[start] = dict(psi=psi.cpu(), z=z.cpu(), z_vjp=z_vjp.cpu(), grad=grad.cpu())
    out["prod"]["z_eval"] = prog.expz(x, th).reshape(S, -1).cpu()          # evaluation plan: readout-only last pass
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def run_case(name: str, jit: bool) -> dict:
    """start -> results of one case on one kernel (computed once, shared by the tests).  Runs everything twice on the
    same program and asserts bitwise-equal <Z> and gradients, and NaN padding behind sample S - 1 left untouched."""
    prog = make_program(sc.BY_NAME[name], torch.device("cuda", 0), jit)
    used = pad_workspaces(prog)
    first = _once(prog, name)
    assert_padding_untouched(prog, used)
    second = _once(prog, name)
    assert_padding_untouched(prog, used)
    for start, r in first.items():
        for key, v in r.items():
            assert torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all(), (start, key)
            if key != "psi":
                assert torch.equal(v, second[start][key]), f"{start}/{key} differs between two runs"
    return first


def errors(name: str, jit: bool) -> dict:
    """start -> key -> max |kernel - float64 reference|."""
    ref = sc.reference(name)
    out = {}
    for start, r in run_case(name, jit).items():
        rr = dict(ref[start], z_eval=ref[start]["z"], z_vjp=ref[start]["z"])
        out[start] = sc.max_errors(r, {k: rr[k] for k in r})
    return out


_RUNS = [(c.name, False) for c in sc.CASES] + [(c.name, True) for c in sc.CASES if c.jit]


@pytest.mark.parametrize("name,jit", _RUNS, ids=[f"{n}-{'jit' if j else 'interp'}" for n, j in _RUNS])
def test_kernel_matches_float64(cuda, name, jit):
    err = errors(name, jit)
    print(name, "jit" if jit else "interp", err)
    for start, e in err.items():
        for key, v in e.items():
            assert v < TOL[key], (start, key, v)
    g = sc.reference(name)["prod"]["grad"].abs().max().item()
    assert g > 1e-2, "degenerate case: the reference gradient is ~0"


@pytest.mark.parametrize("name", [c.name for c in sc.CASES if c.jit])
def test_interpreter_and_per_plan_kernels_agree(cuda, name):
    a, b = run_case(name, False), run_case(name, True)
    for start in a:
        for key, v in a[start].items():
            d = (v - b[start][key]).abs().max().item()
            print(name, start, key, d)
            assert d < TOL[key], (start, key, d)


def test_bf16_storage_tiles(cuda):
    """bf16 storage between the passes of a multi-pass plan with 8-thread tiles: <Z> within the bound of
    test_bf16_state_storage_close_to_fp32 of float64, through packed int32 workspaces, not the fp32 path."""
    case = sc.BF16_CASE
    inp, ref = sc.inputs(case.name), sc.reference(case.name)["prod"]
    x, th, w = inp["x"].to(cuda), inp["theta"].to(cuda), inp["w"].to(cuda)
    b16 = make_program(case, cuda, True, "bf16")
    used = pad_workspaces(b16)
    z16 = b16.expz(x, th).reshape(S, -1).cpu()
    _, zs16 = b16.statevector(x, th)
    zv16, g16 = b16.vjp(x, th, w)
    torch.cuda.synchronize()
    assert_padding_untouched(b16, used)
    assert b16._ws["psi"].dtype == torch.int32 and b16._ws["lam"].dtype == torch.int32
    z32 = make_program(case, cuda, True).expz(x, th).reshape(S, -1).cpu()
    for nm, z in (("expz", z16), ("statevector", zs16.cpu()), ("vjp", zv16.cpu())):
        e = (z.double() - ref["z"]).abs().max().item()
        print(case.name, nm, "bf16 <Z> error", e)
        assert e < 2e-2, (nm, e)
    assert (z32.double() - ref["z"]).abs().max().item() < TOL["z"]
    assert not torch.equal(z16, z32), "bf16 run is bitwise equal to fp32: the storage path was not taken"
    assert torch.isfinite(g16).all()
