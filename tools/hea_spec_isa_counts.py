#!/usr/bin/env python3
"""Instruction counts of the per-plan MFMA pass kernels of one circuit, from their gfx950 assembly (no GPU needed).

Builds the per-plan source of every pass of a program (``hea_spec_source`` with the program's own tables and
``spec_cfg``), cross-compiles each with the options the run-time compiler uses (``-O3 -std=c++17``) and prints per
kernel the static instruction counts by class, the register and LDS budget, spill / scratch sizes and the number of
workgroup barriers.  The pass bodies are straight-line apart from block-bound skips, so the static counts are close to
the per-wave dynamic ones.

    tools/hea_spec_isa_counts.py [--qubits 16] [--layers 3] [--classes 3] [--tile T] [--storage fp16|bf16]
                                 [--lean MASK ...] [--keep DIR]

``--tile 13`` is the retiling the engine picks for steps of few samples (``VQCEngine.fit_tiles``).  ``--lean`` takes one
or more ``QFEDX_HEA_SPEC_LEAN`` masks: one table per mask, then the differences of every later mask against the first.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-S", "--cuda-device-only", "-O3", "-std=c++17", "--offload-arch=gfx950"]
COLS = ["VALU", "v_mov", "v_pk_mul", "SALU", "MFMA", "LDS", "VMEM", "barrier", "VGPR", "SGPR", "LDS_B", "spill", "scratch"]


def classify(op):
    """Instruction class of mnemonic ``op`` (None: a waitcnt / nop / branch / end, counted nowhere)."""
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if op in ("s_barrier",):
        return "barrier"
    if op.startswith(("s_waitcnt", "s_nop", "s_endpgm", "s_branch", "s_cbranch", "s_sleep", "s_setprio", "s_code_end")):
        return None
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    return None


def count(asm, kernel="qfx_hea_spec_pass"):
    """Counts of the kernel's body in the assembly text ``asm`` and its resource notes."""
    m = re.search(r"^%s:.*?^\s*s_endpgm" % re.escape(kernel), asm, re.M | re.S)
    if not m:
        raise RuntimeError("kernel %s not found in the assembly" % kernel)
    out = {k: 0 for k in COLS + ["SMEM"]}
    for line in m.group(0).splitlines()[1:]:
        line = line.split(";")[0].strip()
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        op = line.split()[0]
        cls = classify(op)
        if cls:
            out[cls] += 1
        if op.startswith("v_mov_b32"):
            out["v_mov"] += 1
        if op.startswith("v_pk_mul_f16"):
            out["v_pk_mul"] += 1

    def note(pat, default=0):
        r = re.search(pat, asm)
        return int(r.group(1)) if r else default
    out["VGPR"] = note(r"\.vgpr_count:\s+(\d+)")
    out["SGPR"] = note(r"\.sgpr_count:\s+(\d+)")
    out["LDS_B"] = note(r"\.group_segment_fixed_size:\s+(\d+)")
    out["scratch"] = note(r"\.private_segment_fixed_size:\s+(\d+)")
    out["spill"] = note(r"\.vgpr_spill_count:\s+(\d+)") + note(r"\.sgpr_spill_count:\s+(\d+)")
    return out


def pass_sources(prog):
    """(name, source text) of every pass of ``prog`` that a step can launch per plan."""
    from qfedx_amd.ops._ext import ext
    C = ext()
    for j, ((f, ff), (a, fa)) in enumerate(prog._host_progs):
        if j <= prog.fwd_last and len(f):
            yield "fwd%d" % j, C.hea_spec_source(False, f, ff, prog.spec_cfg(j, False))
        if len(a):
            yield "adj%d" % j, C.hea_spec_source(True, a, fa, prog.spec_cfg(j, True))


def compile_counts(src, workdir, tag):
    from qfedx_amd.ops.statevec_hip import CSRC
    path = os.path.join(workdir, tag + ".hip")
    with open(path, "w") as f:
        f.write(src)
    asm = os.path.join(workdir, tag + ".s")
    subprocess.run(["hipcc", *FLAGS, "-I", CSRC, "-x", "hip", path, "-o", asm], check=True, stderr=subprocess.DEVNULL)
    with open(asm) as f:
        return count(f.read())


def table(title, rows, sign=False):
    print(title)
    print("  %-6s" % "pass" + "".join("%9s" % c for c in COLS))
    for name, r in rows:
        print("  %-6s" % name + "".join(("%+9d" if sign else "%9d") % r[c] for c in COLS))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--qubits", type=int, default=16)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--tile", type=int, default=None, help="forward and adjoint tile bits (default: the engine's)")
    ap.add_argument("--storage", default="fp16", choices=("fp16", "bf16"))
    ap.add_argument("--lean", type=int, nargs="+", default=[0, 1, 7], help="QFEDX_HEA_SPEC_LEAN masks to compile")
    ap.add_argument("--keep", default=None, help="directory that keeps the generated sources and assembly")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from qfedx_amd.models.vqc import VQCSpec
    from qfedx_amd.ops.hea_mfma import HeaMfmaProgram
    spec = VQCSpec(n_qubits=args.qubits, n_layers=args.layers, n_classes=args.classes)
    tiles = {"tile_bits": args.tile, "adj_tile_bits": args.tile} if args.tile else {}
    work = args.keep or tempfile.mkdtemp(prefix="hea_isa_")
    os.makedirs(work, exist_ok=True)
    results = []
    for mask in args.lean:
        prog = HeaMfmaProgram(spec, "cpu", storage=args.storage, use_spec=False, spec_gen=True, spec_lean=mask, **tiles)
        prog.obs_at_load = True
        rows = [(name, compile_counts(src, work, "%s_lean%d" % (name, mask))) for name, src in pass_sources(prog)]
        results.append(rows)
        geo = ", ".join("%s t=%d" % (n, (e.adj_pass if n[0] == "a" else e.fwd_pass).t)
                        for n, e in ((n, prog.passes[int(n[3:])]) for n, _ in rows))
        table("%dq x %dL, %d classes, %s, lean mask %d  (%s)" % (args.qubits, args.layers, args.classes, args.storage, mask,
                                                                 geo), rows)
    for mask, rows in zip(args.lean[1:], results[1:]):
        diff = [(n, {c: r[c] - r0[c] for c in COLS}) for (n, r), (_, r0) in zip(rows, results[0])]
        table("lean mask %d minus mask %d" % (mask, args.lean[0]), diff, sign=True)


if __name__ == "__main__":
    main()
