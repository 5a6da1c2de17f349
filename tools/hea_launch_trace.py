"""Launch traces of the MFMA engine's host (``HeaMfmaProgram``): every native launch a scripted call issues, with its
arguments, for the shapes that reach every branch of the host code.

python tools/hea_launch_trace.py [--out tests/golden/hea_launch_traces.json]

Needs no GPU.  A recorder stands in for ``ext()`` inside ``qfedx_amd.ops.hea_mfma``: it forwards every attribute that
is no launch (``hea_check_ops``, ``hea_spec_key``, ...), hands out consecutive kernel handles instead of compiling
(``hea_spec_prepare``), and records the launch calls WITHOUT running them (``record``).  On a GPU it can forward
everything and record as well (``passthrough``): tests/test_gpu_hea_launch_trace.py shows the device runs what the CPU
trace says.  ``QFX_PKG_ROOT`` selects the tree whose package is traced; tests/golden/hea_launch_traces.json was written
at the commit BEFORE the host was restructured around ``HeaMfmaProgram._launch``, and tests/test_hea_launch_trace.py
holds the working tree to it, call for call.  The tests import the cases and the script from here.

Encoding of a call: [name, positional arguments, keyword arguments].  A tensor is, in this order of preference, the
pass table it IS (``fwd{j}.ops|fidx|fo``, ``adj{j}...``, ``slot_tab``, ``gmeta``), a workspace reference [name, element
offset, numel] found by address in the program's current ``_ws``, or [dtype, shape] ([dtype, [0]] when empty).
``hea_pass`` gains ``fwd{j}`` / ``adj{j}`` after its name and records ``spec`` as true / false (a handle's number
depends on what the process compiled before).  Floats are recorded with ``repr``.
"""
import contextlib
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hea_launch_traces.json")

LAUNCHES = ("hea_pass", "hea_frags", "hea_grad_reduce", "hea_readout_rec", "readout_sum", "readout_ce",
            "readout_noise", "hea_amp_stage", "hea_dp_norm", "hea_dp_reduce", "ps_combine")
PS_BUDGET_MB = "64"
CLEARED_ENV = ("QFEDX_HEA_", "QFEDX_DEBUG", "QFEDX_STAMPS", "QFEDX_EXTRA_HIPFLAGS")      # (the last: spec_cfg reads it)

# Scripted calls (``run_call``).  FULL: every route of a training step, evaluation, VJP; the shorter scripts keep the
# golden file under 200 KB: shapes that differ from a FULL case in one host branch run the calls that reach it.  The
# parameter-shift family dominates the call count: 10q2L_t8 runs all of it, 12q4L_t9 (branches from passes 1..3) and
# 16q3L (parameter rows chunked by the budget) the +pi branches.
SHORT = ("step", "step_noise", "dpsgd", "expz", "vjp")
STEPS = ("step", "step_noise", "dpsgd")
MID = ("step", "step_shared", "step_adam", "step_noise", "dpsgd", "step_private", "expz", "vjp")
FULL = ("step", "step_shared", "step_adam", "step_adam_fed", "step_noise", "dpsgd", "dpsgd_sigma0", "step_private",
        "expz", "expz_chunked", "vjp")

# name: spec (n, L, classes, feature map, entangler), program keywords, K, B, extras (env, split_readout), script
#   10q2L_t8*      two passes; the generating pass 0 on either route; the interpreter everywhere; S = 160 takes the
#                  split route by sample count, and the knob forces it on / off at S = 6
#   10q1L / 12q1L  fwd_last = 0 under J = 2 / 3: identity passes alias the stored output
#   12q4L_t9       four passes
#   12q3L_t8_c8    128 readout partials per sample: the noiseless step runs the readout kernel
#   16q3L*         the headline plan (adjoint on its own 2^13 plan), bf16, the 2^13 forward, the interpreter
#   ring*          ring plans, both adjoint tilings
#   amp*           amplitude programs: staged input, no generating pass
def _case(n, L, tile, script, C=3, fm="ry", ent="chain", K=2, B=3, storage="fp16", use_spec=True, spec_gen=True,
          split=None, env=None):
    return {"spec": (n, L, C, fm, ent), "prog": {"tile_bits": tile, "storage": storage, "use_spec": use_spec,
                                                   "spec_gen": spec_gen},
            "K": K, "B": B, "split": split, "env": env or {}, "script": script}


CASES = {
    "10q2L_t8": _case(10, 2, 8, FULL + ("ps_exact", "ps_shots", "shifted_expz"), spec_gen=False),
    "10q2L_t8_gen": _case(10, 2, 8, SHORT),
    "10q2L_t8_interp": _case(10, 2, 8, ("step", "expz", "vjp"), use_spec=False),
    "10q2L_t8_s160": _case(10, 2, 8, STEPS, K=5, B=32),
    "10q2L_t8_split_on": _case(10, 2, 8, STEPS, split=True),
    "10q2L_t8_split_off": _case(10, 2, 8, STEPS, split=False),
    "10q1L_t8": _case(10, 1, 8, SHORT + ("step_shared",)),
    "12q1L_t8": _case(12, 1, 8, ("step", "dpsgd", "vjp")),
    "12q4L_t9": _case(12, 4, 9, ("step", "vjp", "ps_shots")),
    "12q3L_t8_c8": _case(12, 3, 8, ("step", "step_shared", "step_adam", "step_noise", "expz", "vjp"), C=8),
    "16q3L": _case(16, 3, None, ("step", "dpsgd", "vjp", "ps_shots")),
    "16q3L_bf16": _case(16, 3, None, ("step", "expz"), storage="bf16"),
    "16q3L_t13": _case(16, 3, 13, ("step", "vjp")),
    "16q3L_interp": _case(16, 3, None, ("step", "expz", "vjp"), use_spec=False),
    "ring_10q3L_t8": _case(10, 3, 8, SHORT + ("step_shared", "ps_refused"), ent="ring"),
    "ring_16q3L_adj13": _case(16, 3, None, ("step", "vjp"), ent="ring", env={"QFEDX_HEA_RING_ADJ": "13"}),
    "ring_16q3L_adj14": _case(16, 3, None, ("step", "vjp"), ent="ring", env={"QFEDX_HEA_RING_ADJ": "14"}),
    "amp_8q1L": _case(8, 1, None, MID + ("expz_chunked", "ps_refused", "init_refused"), fm="amplitude"),
    "amp_12q2L_t10": _case(12, 2, 10, ("step", "expz", "vjp"), fm="amplitude"),
}


def pkg_root():
    return os.environ.get("QFX_PKG_ROOT") or ROOT


@contextlib.contextmanager
def case_env(name, jit_cache):
    """The environment a case is traced in: no ``QFEDX_HEA_*`` / debug / stamps knob but the case's own, a 64 MB
    parameter-shift budget, the given JIT cache."""
    saved = dict(os.environ)
    for k in list(os.environ):
        if k.startswith(CLEARED_ENV):
            del os.environ[k]
    os.environ.update(CASES[name]["env"], QFEDX_PS_BUDGET_MB=PS_BUDGET_MB, QFEDX_JIT_CACHE=str(jit_cache))
    try:
        yield
    finally:
        os.environ.clear()
        os.environ.update(saved)


class Recorder:
    """Stands in for the extension module inside ``qfedx_amd.ops.hea_mfma``.  ``passthrough``: launches run as well."""

    def __init__(self, real, passthrough=False):
        self._real, self._passthrough = real, passthrough
        self._handles = 0
        self.prog = None
        self.calls = []

    def _tables(self):
        prog, out = self.prog, {}
        for j, e in enumerate(prog.passes):
            for d, tabs in (("fwd", e[1]), ("adj", e[2])):
                for nm, t in zip(("ops", "fidx", "fo"), tabs):
                    out[id(t)] = f"{d}{j}.{nm}"
        out[id(prog.slot_tab)] = "slot_tab"
        out[id(prog.gmeta)] = "gmeta"
        return out

    def _enc(self, v, tables):
        import torch
        if torch.is_tensor(v):
            if id(v) in tables:
                return tables[id(v)]
            dt = str(v.dtype).replace("torch.", "")
            if v.numel() == 0:
                return [dt, [0]]
            a = v.data_ptr()
            for name, t in self.prog._ws.items():
                if t.data_ptr() <= a < t.data_ptr() + t.numel() * t.element_size():
                    return [name, (a - t.data_ptr()) // t.element_size(), v.numel()]
            return [dt, list(v.shape)]
        if isinstance(v, (list, tuple)):
            return [self._enc(x, tables) for x in v]
        if isinstance(v, float):
            return repr(v)
        return v

    def _record(self, name, a, kw):
        tables = self._tables() if self.prog is not None else {}
        head = [name]
        if name == "hea_pass":
            head.append(tables[id(a[1])].split(".")[0])
            kw = dict(kw, spec=kw.get("spec", -1) >= 0)
        self.calls.append(head + [[self._enc(x, tables) for x in a], {k: self._enc(x, tables) for k, x in sorted(kw.items())}])

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if name == "hea_spec_prepare" and not self._passthrough:
            def prepare(adjoint, ops, fidx, cfg, cache, csrc, arch):
                self._handles += 1
                return self._handles - 1, self._real.hea_spec_key(adjoint, ops, fidx, cfg, csrc, arch)
            return prepare
        if name not in LAUNCHES:
            return real

        def call(*a, **kw):
            self._record(name, a, kw)
            return real(*a, **kw) if self._passthrough else None
        return call


@contextlib.contextmanager
def recording(passthrough=False):
    """Patch ``hea_mfma.ext`` with a recorder for the block."""
    from qfedx_amd.ops import hea_mfma
    real = hea_mfma.ext
    rec = Recorder(real(), passthrough)
    hea_mfma.ext = lambda: rec
    try:
        yield rec
    finally:
        hea_mfma.ext = real


def case_spec(name):
    from qfedx_amd.models.vqc import VQCSpec
    n, L, C, fm, ent = CASES[name]["spec"]
    return VQCSpec(n_qubits=n, n_layers=L, n_classes=C, feature_map=fm, entangler=ent)


def build_program(name, dev):
    from qfedx_amd.ops.hea_mfma import HeaMfmaProgram
    prog = HeaMfmaProgram(case_spec(name), dev, **CASES[name]["prog"])
    if CASES[name]["split"] is not None:
        prog.split_readout = CASES[name]["split"]
    return prog


def case_inputs(name, dev):
    """Inputs of a case, the same on every machine: angles, labels, weights, parameters, raw amplitudes (amplitude
    programs), dL/d<Z>, Philox keys [K, 2]."""
    import torch
    spec, K, B = case_spec(name), CASES[name]["K"], CASES[name]["B"]
    n, C = spec.n_qubits, spec.n_classes
    g = torch.Generator().manual_seed(23)
    x = spec.encode_features(torch.rand(K, B, n, generator=g)).float()
    y = torch.randint(0, C, (K, B), generator=g)
    params = torch.stack([spec.init_params(k) for k in range(K)]).float()
    params = params + 0.3 * torch.randn(params.shape, generator=g)
    init = torch.rand(K, B, (1 << n) - 3, generator=g) if spec.amplitude else None
    w = torch.randn(K, B, C, generator=g)
    inp = {"x": x, "y": y, "wmask": torch.full((K, B), 1.0 / B), "params": params.contiguous(), "init": init, "w": w,
           "keys": torch.arange(1, 2 * K + 1).reshape(K, 2)}
    return {k: (v.to(dev) if v is not None else None) for k, v in inp.items()}


class Noise:
    p01, p10, shots = 0.01, 0.02, 100


class StandInOptimizer:
    """``fused_adam`` of the shapes ``hea_grad_reduce`` checks: (m, v [K, P], t_in, t_out, active [K]), four floats."""

    def fused_adam(self, p, active):
        import torch
        K = p.shape[0]
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=p.device)
        return [z(K, p.shape[1]), z(K, p.shape[1]), z(K), z(K), active.float().contiguous()], [0.05, 0.9, 0.999, 1e-8]


def fed_tail(p):
    """A FedAvg tail of dummy tensors of the shapes ``hea_grad_reduce`` checks (9 tensors, 2 norm slots)."""
    import torch
    P, K, dev = p.shape[1], p.shape[0], p.device
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    return {"fed": [z(P + 8, torch.int64), z(P, torch.float32), z(P, torch.uint8), torch.ones(K, dtype=torch.float64,
                                                                                            device=dev)]
            + [z(4, torch.float32) for _ in range(4)] + [z(1, torch.int32)], "wrap": True, "n_norms": 2}


def run_call(prog, name, what, inp):
    """One scripted call -> its result (tensors or a refusal's message)."""
    import torch
    spec = prog.spec
    K, B = CASES[name]["K"], CASES[name]["B"]
    x, y, wm, params, init, w, keys = (inp[k] for k in ("x", "y", "wmask", "params", "init", "w", "keys"))
    theta = params[:, :spec.n_theta]

    def step(**kw):
        return prog.loss_and_grads(x, y, wm, params, spec, init=init, **kw)

    if what == "step":
        return step()
    if what == "step_shared":
        job = prog.prologue_frag_job()
        return step(shared_frags=job[1] if job else None)
    if what in ("step_adam", "step_adam_fed"):
        active = torch.ones(K, device=params.device)
        return step(fused_opt=(StandInOptimizer(), active), fed_tail=fed_tail(params) if what == "step_adam_fed" else None)
    if what == "step_noise":
        return step(noise=Noise(), keys=keys, step=3)
    if what in ("dpsgd", "dpsgd_sigma0"):
        return step(dpsgd={"clip": 1.0, "sigma": 0.0 if what == "dpsgd_sigma0" else 1.5, "keys": keys, "step": 2,
                           "lot": float(B)})
    if what == "step_private":
        with prog.private_workspace({}):
            return step()
    if what == "expz":
        return prog.expz(x, theta, init=init)
    if what == "expz_chunked":
        os.environ["QFEDX_PS_BUDGET_MB"] = "0"                 # below one client's states: one client per launch
        saved, prog._ps_budget = prog._ps_budget, None         # (the budget is read once and kept)
        try:
            return prog.expz(x, theta, init=init)
        finally:
            os.environ["QFEDX_PS_BUDGET_MB"] = PS_BUDGET_MB
            prog._ps_budget = saved
    if what == "vjp":
        return prog.vjp(x, theta, w, init=init)
    if what == "ps_exact":
        return prog.param_shift(x, params, w, exact_only=True)
    if what == "ps_shots":
        return prog.param_shift(x, params, w, noise=Noise(), keys=keys, step=1)
    if what == "shifted_expz":
        return prog.shifted_expz(x, params)
    if what in ("ps_refused", "init_refused"):
        try:
            if what == "ps_refused":
                prog.param_shift(x, params, w, exact_only=True)
            else:
                prog.expz(x, theta)
        except ValueError as e:
            return str(e)
        raise AssertionError(f"{name}: {what} did not raise")
    raise KeyError(what)


def clone(res):
    """A scripted call's tensors, copied (a step's ``expz`` is a workspace view the next call overwrites)."""
    import torch
    if torch.is_tensor(res):
        return res.clone()
    if isinstance(res, dict):
        return {k: clone(v) for k, v in res.items()}
    if isinstance(res, (list, tuple)):
        return [clone(v) for v in res]
    return res


def tensors(res):
    """The tensors of a scripted call's result, in a fixed order."""
    import torch
    if torch.is_tensor(res):
        return [res]
    if isinstance(res, dict):
        return [t for k in sorted(res) for t in tensors(res[k])]
    if isinstance(res, (list, tuple)):
        return [t for v in res for t in tensors(v)]
    return []


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def header(prog, name):
    S = CASES[name]["K"] * CASES[name]["B"]
    J = prog.n_passes
    tabs = {}
    for j, e in enumerate(prog.passes):
        for d, t in (("fwd", e[1]), ("adj", e[2])):
            tabs[f"{d}{j}"] = [_sha(v) for v in t]
    return {"n_passes": J, "fwd_last": prog.fwd_last, "tile_bits": [e[0].t for e in prog.passes],
            "adj_tile_bits": [e[3].t for e in prog.passes], "n_regions": list(prog.n_regions),
            "n_gradops": prog.n_gradops, "slab_tiles": prog.slab_tiles, "grad_cover_exact": bool(prog.grad_cover_exact),
            "n_slots": prog.n_slots,
            "spec_cfg": {f"{'adj' if a else 'fwd'}{j}": prog.spec_cfg(j, a) for a in (False, True) for j in range(J)},
            "tables": tabs, "slot_tab": _sha(prog.slot_tab), "gmeta": _sha(prog.gmeta),
            "spec_passes": prog.spec_passes(), "spec_passes_S": prog.spec_passes(samples=S),
            "readout_mode_S": prog.readout_mode(S)}


def trace_case(name, dev="cpu", passthrough=False, script=None, jit_cache=None):
    """-> ({"header", "calls": {scripted call: [launches]}, "counters": {scripted call: [spec, interp]},
    "refused": {...}}, results per scripted call, the program)."""
    import tempfile
    with contextlib.ExitStack() as stack:
        if jit_cache is None:
            jit_cache = stack.enter_context(tempfile.TemporaryDirectory())
        stack.enter_context(case_env(name, jit_cache))
        rec = stack.enter_context(recording(passthrough))
        prog = build_program(name, dev)
        rec.prog = prog
        out = {"header": header(prog, name), "calls": {}, "counters": {}, "refused": {}}
        results = {}
        inp = case_inputs(name, dev)
        for what in (script or CASES[name]["script"]):
            rec.calls = []
            res = run_call(prog, name, what, inp)
            if isinstance(res, str):
                out["refused"][what] = res
            else:
                results[what] = clone(res)
            out["calls"][what] = rec.calls
            out["counters"][what] = [prog.spec_launches, prog.interp_launches]
    return out, results, prog


def dumps(table):
    """Sorted keys, one launch per line."""
    lines = ["{"]
    names = sorted(table)
    for i, name in enumerate(names):
        c = table[name]
        lines.append(f' {json.dumps(name)}: {{')
        for key in ("counters", "header", "refused"):
            lines.append(f'  {json.dumps(key)}: {json.dumps(c[key], sort_keys=True, separators=(",", ":"))},')
        lines.append('  "calls": {')
        whats = sorted(c["calls"])
        for k, what in enumerate(whats):
            lines.append(f'   {json.dumps(what)}: [')
            calls = c["calls"][what]
            lines += [f'    {json.dumps(call, sort_keys=True, separators=(",", ":"))}{"," if m + 1 < len(calls) else ""}'
                      for m, call in enumerate(calls)]
            lines.append("   ]" + ("," if k + 1 < len(whats) else ""))
        lines.append("  }")
        lines.append(" }" + ("," if i + 1 < len(names) else ""))
    lines.append("}")
    return "\n".join(lines) + "\n"


def main():
    sys.path.insert(0, pkg_root())
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    import qfedx_amd
    print("package:", os.path.dirname(qfedx_amd.__file__))
    table = {}
    for name in CASES:
        table[name] = json.loads(json.dumps(trace_case(name)[0]))
        print(name, {k: len(v) for k, v in table[name]["calls"].items()}, flush=True)
    text = dumps(table)
    assert json.loads(text) == table
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print("wrote", out, len(text), "bytes")


if __name__ == "__main__":
    main()
