"""The two MPS kernels (csrc/mps_chain.hip, csrc/mps_mpo.hip) at their shape edges against float64.

Every case of tests/mps_cases.py runs on its kernel through the wrappers of ops/mps_hip.py: n = 2 and 3, C = 1 and 8,
repeated readout qubits, qmax = 0, batches that split a block between clients, 16-wide bonds on two qubits, four
pass-throughs, idle qubits, every fixed gate and trajectory Pauli between two rotations, 64 rotations on one qubit.
References are float64 (the column oracle / the complex128 dense statevector) on the same float32 inputs;
tests/test_mps_cases.py proves on the CPU what each case reaches, that the references agree with the dense
statevector and that the complex64 dense executor stays within half of every bound used here.  Bounds are the
project's existing ones (tests/test_gpu_mps_chain.py, tests/test_gpu_mps.py), held against float64: <Z> 2e-5, MPO
per-gate dang 5e-5, chain per-client gradient sums 1e-4, fused loss rtol 1e-4 / atol 1e-5, fused gradients 1e-4,
dL/dlogit 2e-5, hits exact.  Each case runs twice on the same program object on NaN-filled scratch sized for one
more sample: results must be finite and bitwise equal, the padding untouched.  Measured errors:
profiles/mps_edges_err_table.txt (tools/mps_err_table.py)."""
import functools

import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops._ext import ext
from qfedx_amd.ops.mps_hip import MpsChainProgram
from qfedx_amd.quantum.mps import MPSProgram
from qfedx_amd.quantum.mps_mpo import ROTATIONS
from tests import mps_cases as mc

pytestmark = pytest.mark.gpu

NAN = float("nan")
_EMPTY = torch.zeros(0)
CHAIN_IDS = [c.name for c in mc.CHAIN_CASES]
FUSED_IDS = [c.name for c in mc.FUSED_CASES]
MPO_IDS = [c.name for c in mc.MPO_CASES]


def _dev():
    return torch.device("cuda", 0)


def _nan(numel: int) -> torch.Tensor:
    return torch.full((numel,), NAN, dtype=torch.float32, device=_dev())


def pad_scratch(prog, S: int, per_rp: int, per_ro: int) -> dict:
    """Replace the program's right-environment scratch by NaN-filled buffers sized for S + 1 samples."""
    bufs = {"rp": _nan((S + 1) * per_rp), "ro": _nan((S + 1) * per_ro)}
    prog._ws.update(bufs)
    return bufs


def assert_scratch_padding(prog, bufs: dict, S: int) -> None:
    for name, t in bufs.items():
        assert prog._ws[name] is t, f"{name} scratch was reallocated"
        per = t.numel() // (S + 1)
        assert bool(t[S * per:].isnan().all()), f"{name}: write past sample S - 1"


def assert_twice(run) -> dict:
    """Results of ``run()`` (name -> tensor, on the CPU), run twice: finite and bitwise equal."""
    first, second = run(), run()
    for k, v in first.items():
        assert bool(torch.isfinite(v).all()), f"{k} is not finite"
        assert torch.equal(v, second[k]), f"{k} differs between two runs"
    return first


def same_sums(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Sums over a client's B <= 5 samples formed on the device and on the host: equal up to the order of at most five
    fp32 additions of O(1) terms (a few ulp), far below any bound against float64."""
    return float((a - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ chain kernel
@functools.lru_cache(maxsize=None)
def run_chain(name: str) -> dict:
    c, i = mc.CHAIN_BY_NAME[name], mc.chain_inputs(name)
    dev = _dev()
    prog = MpsChainProgram(c.spec(), dev)
    bufs = pad_scratch(prog, c.S, c.n * 128, (max(c.readout) + 1) * 128)
    x, th, w = i["xarg"].to(dev), i["targ"].to(dev), i["w"].to(dev)

    def run():
        z = prog.expz(x, th)
        z_g, g = prog._run(x, th, w)
        out = dict(z=z.reshape(c.S, c.C).cpu(), z_grad=z_g.reshape(c.S, c.C).cpu(), grad_s=g.reshape(c.S, -1).cpu(),
                   grad=prog.grads(x, th, w).cpu())
        assert_scratch_padding(prog, bufs, c.S)
        return out
    out = assert_twice(run)
    assert same_sums(out["grad"], out["grad_s"].reshape(c.K, c.B, -1).sum(1))
    return out


def chain_errors(name: str) -> dict:
    ref, out = mc.chain_reference(name), run_chain(name)
    return {k: mc.within(b, out[k], ref[r]) + (mc.TOL[b],)
            for k, r, b in (("z", "z", "z"), ("z_grad", "z", "z"), ("grad", "grad", "grad"))}


@pytest.mark.parametrize("name", CHAIN_IDS)
def test_chain_kernel_matches_float64(cuda, name):
    err = chain_errors(name)
    print(name, {k: f"{e:.2e}" for k, (e, _, _) in err.items()})
    for k, (e, ok, _) in err.items():
        assert ok, (k, e)


def fused_raw(prog: MpsChainProgram, c, i: dict, y: torch.Tensor, pad: int = 0) -> dict:
    """The fused launch as ``MpsChainProgram.train`` issues it, with outputs allocated for S + pad samples (NaN)."""
    dev, S, C = prog.device, c.S, c.C
    out = dict(z=_nan((S + pad) * C), dl=_nan((S + pad) * C), lossv=_nan(S + pad), hitv=_nan(S + pad),
               g=_nan((S + pad) * 2 * c.n * c.L))
    ext().mps_chain(i["x"].reshape(S, c.n).to(dev), i["params"].to(dev), c.B, c.n, c.L, prog.feature, prog.readout,
                    _EMPTY, out["z"], out["g"], prog._buf("rp", S * c.n * 128),
                    prog._buf("ro", S * (max(c.readout) + 1) * 128), y.reshape(S).to(dev),
                    i["wmask"].reshape(S).to(dev), prog.n_theta, out["dl"], out["lossv"], out["hitv"])
    return out


@functools.lru_cache(maxsize=None)
def run_fused(name: str) -> dict:
    c, i, y = mc.CHAIN_BY_NAME[name], mc.chain_inputs(name), mc.fused_labels(name)
    dev = _dev()
    prog = MpsChainProgram(c.spec(), dev)
    bufs = pad_scratch(prog, c.S, c.n * 128, (max(c.readout) + 1) * 128)
    x, p, yd, wm = i["x"].to(dev), i["params"].to(dev), y.to(dev), i["wmask"].to(dev)

    def run():
        loss, grad, correct, z = prog.train(x, p, yd, wm)
        raw = fused_raw(prog, c, i, y)
        out = dict(loss=loss.cpu(), grad=grad.cpu(), correct=correct.cpu(), z=z.reshape(c.S, c.C).cpu(),
                   dl=raw["dl"].reshape(c.S, c.C).cpu(), lossv=raw["lossv"].cpu(), hitv=raw["hitv"].cpu(),
                   z_raw=raw["z"].reshape(c.S, c.C).cpu(), g_raw=raw["g"].reshape(c.S, -1).cpu())
        assert_scratch_padding(prog, bufs, c.S)
        return out
    out = assert_twice(run)
    # train() is the same launch plus sums over each client's samples
    K, B = c.K, c.B
    dlk, zk = out["dl"].reshape(K, B, -1), out["z_raw"].reshape(K, B, -1)
    assert torch.equal(out["z"], out["z_raw"])
    assert same_sums(out["loss"], out["lossv"].reshape(K, B).sum(1))
    assert torch.equal(out["correct"], out["hitv"].reshape(K, B).sum(1))
    assert same_sums(out["grad"], torch.cat([out["g_raw"].reshape(K, B, -1).sum(1), (dlk * zk).sum(1), dlk.sum(1)], -1))
    return out


def fused_errors(name: str) -> dict:
    ref, out = mc.fused_reference(name), run_fused(name)
    return {k: mc.within(b, out[k], ref[k]) + (mc.TOL.get(b, "rtol 1e-4 + 1e-5"),) for k, b in mc.FUSED_KEYS.items()}


@pytest.mark.parametrize("name", FUSED_IDS)
def test_fused_train_matches_float64(cuda, name):
    err = fused_errors(name)
    print(name, {k: f"{e:.2e}" for k, (e, _, _) in err.items()})
    for k, (e, ok, _) in err.items():
        assert ok, (k, e)
    ref, out = mc.fused_reference(name), run_fused(name)
    assert torch.equal(out["hitv"].double(), ref["hitv"])                # every sample, none left out
    assert torch.equal(out["correct"].double(), ref["correct"].double())


def test_chain_binding_outputs_behind_the_batch_stay_untouched(cuda):
    """The fused launch with z, grad, dl, lossv, hitv allocated for S + 1 samples: sample S is never written."""
    c = mc.CHAIN_BY_NAME["fused_n10_L3_c8"]
    prog = MpsChainProgram(c.spec(), cuda)
    raw = fused_raw(prog, c, mc.chain_inputs(c.name), mc.fused_labels(c.name), pad=1)
    torch.cuda.synchronize()
    good = run_fused(c.name)
    for k, key in (("z", "z_raw"), ("dl", "dl"), ("lossv", "lossv"), ("hitv", "hitv"), ("g", "g_raw")):
        per = raw[k].numel() // (c.S + 1)
        assert bool(raw[k][c.S * per:].isnan().all()), f"{k}: write past sample S - 1"
        assert torch.equal(raw[k][: c.S * per].cpu(), good[key].reshape(-1)), k


def test_chain_empty_batch(cuda):
    spec = VQCSpec(4, 2, 3)
    prog = MpsChainProgram(spec, cuda)
    x, th = torch.zeros(0, 3, 4, device=cuda), torch.zeros(0, spec.n_theta, device=cuda)
    assert prog.expz(x, th).shape == (0, 3, 3)
    assert prog.grads(x, th, torch.zeros(0, 3, 3, device=cuda)).shape == (0, spec.n_theta)
    loss, grad, correct, z = prog.train(x, torch.zeros(0, spec.n_params, device=cuda),
                                        torch.zeros(0, 3, dtype=torch.long, device=cuda), torch.zeros(0, 3, device=cuda))
    assert loss.shape == (0,) and grad.shape == (0, spec.n_params) and correct.shape == (0,) and z.shape == (0, 3, 3)


def _chain_call(dev, n=4, L=2, readout=(0, 1), K=3, B=3, **over):
    """A valid gradient-mode call of the chain binding on NaN outputs; ``over`` replaces arguments by name."""
    S, C = K * B, len(readout)
    a = dict(x=torch.zeros(S, n, device=dev), theta=torch.zeros(K, 2 * n * L, device=dev), spc=B, n=n, L=L, feature=0,
             readout=list(readout), w=torch.ones(S, C, device=dev), z=_nan(S * C), grad=_nan(S * 2 * n * L),
             rp=_nan(S * n * 128), ro=_nan(S * (max(readout) + 1) * 128))
    a.update(over)
    return a


def _refused(fn, args: dict, match: str, outs=("z", "grad")):
    with pytest.raises(ValueError, match=match):
        fn(**args)
    torch.cuda.synchronize()
    for k in outs:
        assert bool(args[k].isnan().all()), f"{k} was written by a refused call"


def test_chain_binding_refuses_bad_arguments(cuda):
    f = ext().mps_chain
    f(**_chain_call(cuda))                                                           # the baseline itself is accepted
    _refused(f, _chain_call(cuda, readout=(0, 4)), "readout qubit out of range")    # qubit = n
    S = 9
    _refused(f, _chain_call(cuda, readout=(0, 1, 2, 3, 0, 1, 2, 3, 0), w=torch.ones(S, 9, device=cuda), z=_nan(S * 9)),
             "1..8 readout qubits")
    _refused(f, _chain_call(cuda, L=4, theta=torch.zeros(3, 32, device=cuda), grad=_nan(S * 32)), "layer range")
    _refused(f, _chain_call(cuda, spc=2), "clients x spc")
    _refused(f, _chain_call(cuda, x=torch.zeros(S, 8, device=cuda)[:, ::2]), "x: expected a contiguous")
    _refused(f, _chain_call(cuda, rp=_nan(S * 4 * 128 - 1)), "rp: too small")
    _refused(f, _chain_call(cuda, ro=_nan(S * 2 * 128 - 1)), "ro: too small")
    fused = dict(w=_EMPTY, theta=torch.zeros(3, 16 + 4, device=cuda), y=torch.zeros(S, dtype=torch.long, device=cuda),
                 wts=torch.ones(S, device=cuda), dl=_nan(S * 2), lossv=_nan(S), hitv=_nan(S))
    f(**_chain_call(cuda, ro_off=16, **fused))
    fused.update(dl=_nan(S * 2), lossv=_nan(S), hitv=_nan(S))
    _refused(f, _chain_call(cuda, ro_off=17, **fused), "outside the theta rows", ("z", "grad", "dl", "lossv", "hitv"))
    with pytest.raises(ValueError, match="1..3 layers"):
        MpsChainProgram(VQCSpec(4, 4, 2), cuda)


# ------------------------------------------------------------------------------------------------ MPO kernel
def mpo_program(name: str):
    c = mc.MPO_BY_NAME[name]
    ops, coef = c.build()[:2]
    hip = MPSProgram(ops, coef, c.n, _dev()).hip_program()
    assert hip is not None, f"{name}: the MPO kernel refused the program"
    return hip


@functools.lru_cache(maxsize=None)
def run_mpo(name: str) -> dict:
    c, i = mc.MPO_BY_NAME[name], mc.mpo_inputs(name)
    dev = _dev()
    hip = mpo_program(name)
    assert torch.equal(hip.mask.cpu(), i["mask"])
    bufs = pad_scratch(hip, c.S, c.n * 512, (max(c.readout) + 1) * 512)
    ang, w = i["ang"].to(dev), i["w"].to(dev)

    def run():
        z, none = hip.run(ang, c.readout)
        z_g, dang = hip.run(ang, c.readout, w)
        assert none is None
        assert_scratch_padding(hip, bufs, c.S)
        return dict(z=z.cpu(), z_grad=z_g.cpu(), dang=dang.cpu())
    return assert_twice(run)


def mpo_errors(name: str) -> dict:
    ref, out = mc.mpo_reference(name), run_mpo(name)
    return {k: mc.within(b, out[k], ref[r]) + (mc.TOL[b],)
            for k, r, b in (("z", "z", "z"), ("z_grad", "z", "z"), ("dang", "dang", "dang"))}


@pytest.mark.parametrize("name", MPO_IDS)
def test_mpo_kernel_matches_float64(cuda, name):
    err = mpo_errors(name)
    print(name, {k: f"{e:.2e}" for k, (e, _, _) in err.items()})
    for k, (e, ok, _) in err.items():
        assert ok, (k, e)


def test_mpo_all_64_rotations_of_one_qubit(cuda):
    """Every one of the 64 rotations on qubit 1 has a derivative well above the bound in the float64 reference
    (tests/test_mps_cases.py) and the kernel's matches it."""
    ref, out, mask = mc.mpo_reference("maxpg64")["dang"], run_mpo("maxpg64")["dang"], mc.mpo_inputs("maxpg64")["mask"]
    on_q1 = torch.tensor([k in ROTATIONS and q == 1 for k, q, _, _ in mc.ops_list(mc.maxpg64()[0])])
    assert int(on_q1.sum()) == 64 and bool(mask[on_q1].all())
    assert bool((out[:, on_q1] != 0).all())
    err = (out.double() - ref).abs()[:, on_q1].max(0).values
    assert float(err.max()) < mc.TOL["dang"], err


def test_mpo_binding_outputs_behind_the_batch_stay_untouched(cuda):
    """z and dang allocated for S + 1 samples and NaN-filled: the kernel writes the rotations of S samples only."""
    name = "uneven_bonds"
    c, i, hip = mc.MPO_BY_NAME[name], mc.mpo_inputs(name), mpo_program(name)
    S, C, G = c.S, len(c.readout), hip.G
    z, dang = _nan((S + 1) * C), _nan((S + 1) * G)
    t, h = hip.tab, hip.tab_host
    ext().mps_mpo(i["ang"].to(cuda), t["gkind"], t["events"], t["sinfo"], t["nbits"], h["sinfo"], h["nbits"],
                  list(c.readout), i["w"].to(cuda), z, dang, hip._buf("rp", S * c.n * 512),
                  hip._buf("ro", S * (max(c.readout) + 1) * 512))
    torch.cuda.synchronize()
    good = run_mpo(name)
    assert bool(z[S * C:].isnan().all()) and bool(dang[S * G:].isnan().all())
    assert torch.equal(z[: S * C].cpu().reshape(S, C), good["z_grad"])
    d = dang[: S * G].cpu().reshape(S, G)
    rot = torch.tensor([k in ROTATIONS for k in h["gkind"].tolist()])
    assert bool(d[:, ~rot].isnan().all()) and bool(torch.isfinite(d[:, rot]).all())     # others untouched
    assert torch.equal(torch.where(i["mask"], d, torch.zeros_like(d)), good["dang"])


def test_mpo_empty_batch(cuda):
    hip = mpo_program("ring4")
    z, dang = hip.run(torch.zeros(0, hip.G, device=cuda), [0, 1], torch.zeros(0, 2, device=cuda))
    assert z.shape == (0, 2) and dang.shape == (0, hip.G)
    assert hip.run(torch.zeros(0, hip.G, device=cuda), [3])[0].shape == (0, 1)


def test_mpo_refuses_bad_arguments(cuda):
    name = "ring4"
    c, i, hip = mc.MPO_BY_NAME[name], mc.mpo_inputs(name), mpo_program(name)
    ang, w = i["ang"].to(cuda), i["w"].to(cuda)
    S, G = ang.shape
    with pytest.raises(ValueError, match="angles"):
        hip.run(ang[:, :-1], [0])
    for ro in ([], list(range(4)) * 2 + [0]):
        with pytest.raises(ValueError, match="1..8 qubits"):
            hip.run(ang, ro)
    t, h = hip.tab, hip.tab_host

    def call(readout=(0, 1), **over):
        C = len(readout)
        a = dict(ang=ang, gkind=t["gkind"], events=t["events"], sinfo=t["sinfo"], nbits=t["nbits"],
                 sinfo_host=h["sinfo"], nbits_host=h["nbits"], readout=list(readout),
                 w=torch.ones(S, max(C, 1), device=cuda), z=_nan(S * max(C, 1)), dang=_nan(S * G),
                 rp=_nan(S * c.n * 512), ro=_nan(S * c.n * 512))
        a.update(over)
        return a
    f = ext().mps_mpo
    f(**call())                                                                      # the baseline itself is accepted
    _refused(f, call(ang=ang[:, :-1].contiguous()), "table shapes", ("z", "dang"))
    _refused(f, call(readout=()), "1..8 readout qubits", ("z", "dang"))
    _refused(f, call(readout=(0, 1, 2, 3, 0, 1, 2, 3, 0)), "1..8 readout qubits", ("z", "dang"))
    _refused(f, call(readout=(0, 4)), "readout qubit out of range", ("z", "dang"))
    wide = h["nbits"].clone()
    wide[1] = 5
    _refused(f, call(nbits_host=wide), "bond over 16", ("z", "dang"))
    _refused(f, call(rp=_nan(S * c.n * 512 - 1)), "rp: too small", ("z", "dang"))


def test_simulator_vjp_shared_parameter_and_constant_rotation(cuda):
    """``Simulator(backend="mps")`` on the MPO kernel against the float64 dense ``Simulator.vjp``: slot gradients sum
    two gates of different coefficient, the constant-angle rotations are masked out of dang."""
    from qfedx_amd.quantum.simulator import Simulator
    circ, i = mc.shared_parameter_circuit(), mc.sim_inputs()
    sim = Simulator(circ, mc.SIM_READOUT, backend="mps", device=cuda)
    hip = sim.prog.hip_program()
    assert hip is not None and int(hip.mask.sum()) == 8 and hip.G - int(hip.mask.sum()) == 6
    z, g = sim.vjp(i["v"].to(cuda), i["w"].to(cuda))
    z2, g2 = sim.vjp(i["v"].to(cuda), i["w"].to(cuda))
    z_ref, g_ref = Simulator(circ, mc.SIM_READOUT).vjp(i["v"], i["w"])
    assert torch.equal(z, z2) and torch.equal(g, g2) and hip.launches == 4
    ez, eg = float((z.cpu() - z_ref).abs().max()), float((g.cpu() - g_ref).abs().max())
    print("simulator", ez, eg)
    assert ez < mc.TOL["z"] and eg < mc.TOL["sim_grad"]
    assert float(g_ref.abs().max()) > 1e-2
