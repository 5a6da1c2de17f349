"""Floating-point dataflow of the layer-1 generation block of the MFMA forward pass kernels, read from gfx950 assembly.

python tools/hea_gen_isa.py asm  SRC.hip OUT.s [-I DIR]         compile one source to device assembly (hipcc -S)
python tools/hea_gen_isa.py spec OUT.hip [--retile 13]           write the per-plan text of the headline's pass 0
python tools/hea_gen_isa.py show FILE.s [KERNEL_SUBSTRING]       per forward kernel: the block's values and resources
python tools/hea_gen_isa.py diff A.s B.s                         compare kernel by kernel (same mangled name)
python tools/hea_gen_isa.py same FILE.s SUB_A FILE2.s SUB_B      compare two named kernels (interpreter / per-plan)

The ahead-of-time build compiles the block's plain products and its compiler chooses which product of a sum it fuses;
the per-plan build (QFX_HEA_SPEC) names every rounding in the source, in those forms.  This tool reads both choices back
from the assembly, so that a compiler which decides differently is seen here and not first in the bits.

The block (hea_mfma.hip fwd_pass, `if (a.gen)`, and l1_factor) is straight-line code with a few predicated regions, so
it is evaluated symbolically in program order: a register holds an expression over loads, wave shuffles and v_sin /
v_cos; v_mul / v_fma / v_fmac / v_pk_mul / v_pk_fma (with their op_sel and neg modifiers) build on them, products
written with sorted operands.  A value is reported where it leaves the block: an LDS store of an fp32 value (layer-1
factors, outer product, half-index tables) or a conversion to the storage format (the quads).  Two kernels whose
reported values are equal as multisets round the same products and fuse the same ones, whatever their registers,
packing (v_pk_* or scalar) and scheduling.  LDS loads are named by the array they read (arrays ranked by address).
The kernel descriptor's float modes and resources are printed with it.
"""
import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLAGS = ["-S", "--cuda-device-only", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-gpu-rdc", "-munsafe-fp-atomics"]
# bytes of the LDS arrays the block reads, in address order (the allocator places the larger arrays first): tabA, tabB,
# wv, outer_s.  A per-plan kernel folds constant indices into the address, so an array is read at several bases.
GEN_ARRAYS = (1024, 1024, 512, 8)
KERNEL_RE = re.compile(r"^(_ZN\S*hea_fwd_kernel\S*|qfx_hea_spec_pass):")


def kernels(path):
    """{name: (body lines, descriptor dict)} of the forward pass kernels in an assembly file."""
    lines = open(path).read().split("\n")
    out = {}
    i = 0
    while i < len(lines):
        m = KERNEL_RE.match(lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        j = i + 1
        while j < len(lines) and not lines[j].startswith("\t.amdhsa_kernel"):
            j += 1
        desc = {}
        k = j
        while k < len(lines) and not lines[k].startswith("\t.end_amdhsa_kernel"):
            t = lines[k].split()
            if len(t) == 2 and t[0].startswith(".amdhsa_"):
                desc[t[0][8:]] = t[1]
            k += 1
        while k < len(lines) and not lines[k].startswith("; WaveLimiterHint"):
            m2 = re.match(r"; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", lines[k])
            if m2:
                desc[m2.group(1)] = m2.group(2)
            k += 1
        out[name] = (lines[i + 1:j], desc)
        i = k
    return out


class Sym:
    """Interned expressions; an expression is known by a short hash of its tree."""

    def __init__(self):
        self.text = {}

    def node(self, op, *kids):
        h = hashlib.sha1((op + "(" + ",".join(kids) + ")").encode()).hexdigest()[:12] if kids else op
        if kids:
            self.text[h] = (op, kids)
        return h

    def show(self, h, depth=2):
        if h not in self.text:
            return h
        op, kids = self.text[h]
        if depth == 0:
            return "#" + h[:6]
        return op + "(" + ", ".join(self.show(k, depth - 1) for k in kids) + ")"

    def fp(self, h):
        if h not in self.text:
            return False
        op, kids = self.text[h]
        return op in ("mul", "fma", "fnma") or (op in ("sel", "neg") and any(self.fp(k) for k in kids))


def regs(tok):
    """'v[2:3]' -> ['v2', 'v3'];  'v5' -> ['v5'];  anything else -> [tok]"""
    m = re.match(r"^(-?)([vsa])\[(\d+):(\d+)\]$", tok)
    if m:
        return [m.group(1) + m.group(2) + str(i) for i in range(int(m.group(3)), int(m.group(4)) + 1)]
    return [tok]


def lit(tok):
    try:
        return int(tok, 0)
    except ValueError:
        return None


def evaluate(body, perm=None, taken=False):
    """-> (sorted list of (kind, hash), Sym, fp instruction counts, LDS arrays read).  ``perm``: rename array r to
    perm[r].  ``taken``: a select between a product and the value it would replace is read as the product (every
    predicated table factor applied), so that an interpreter kernel compares with a per-plan kernel whose predicates
    folded at compile time - true for tiles of 2^14 and 2^13 amplitudes, where both half tables hold >= 6 factors."""
    S = Sym()
    R = {}          # register -> expression
    base = {}       # register -> LDS array base its integer value carries (address arithmetic)
    loads = []      # (base, [dest registers]) in program order, named once every base is known
    outs, counts = [], {}
    label_at = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label_at[m.group(1)] = i

    def val(tok):
        minus = tok.startswith("-")
        t = tok[1:] if minus else tok
        if re.match(r"^[vsa]\d+$", t):
            e = R.get(t)
            if e is None:
                e = "S" if t[0] == "s" else "V"
        elif t in ("vcc", "exec", "vcc_lo", "vcc_hi"):
            e = "S"
        else:
            e = "k" + t
        return neg(e) if minus else e

    def unneg(e):
        """(expression without its outer negations, their parity)"""
        n = 0
        while e in S.text and S.text[e][0] == "neg":
            e, n = S.text[e][1][0], n + 1
        return e, n & 1

    def neg(e):
        u, n = unneg(e)
        return u if n else S.node("neg", u)

    # signs are exact: a product's sign is written once, outside it (fma: in its name), so that equal roundings compare
    # equal wherever the compiler put the negations
    def mul(a, b):
        (a, na), (b, nb) = unneg(a), unneg(b)
        e = S.node("mul", *sorted((a, b)))
        return neg(e) if na ^ nb else e

    def fma(a, b, c):
        (a, na), (b, nb) = unneg(a), unneg(b)
        return S.node("fnma" if na ^ nb else "fma", *sorted((a, b)), c)

    def mods(rest):
        d = {}
        for k, v in re.findall(r"(op_sel|op_sel_hi|neg_lo|neg_hi):\[([\d,]+)\]", rest):
            d[k] = [int(x) for x in v.split(",")]
        return d

    def step(l, idx):
        if idx in seen_line:
            record = False
        else:
            record = True
            seen_line.add(idx)
        t = l.strip()
        if not t or t[0] in ";.":
            return
        t = t.split(";")[0].strip()
        op, _, rest = t.partition(" ")
        args = [a.strip() for a in re.split(r",\s*(?![^\[]*\])", rest.split(" op_sel")[0].split(" neg_")[0].split(" offset:")[0])] if rest else []
        off = re.search(r"offset:(\d+)", rest)
        off = int(off.group(1)) if off else 0
        md = mods(rest)
        if op.startswith(("v_mul_f32", "v_fma_f32", "v_fmac_f32", "v_pk_mul_f32", "v_pk_fma_f32", "v_add_f32", "v_sub_f32",
                          "v_pk_add_f32", "v_mac_f32", "v_mad_f32")):
            counts[op.split("_e")[0]] = counts.get(op.split("_e")[0], 0) + 1
        if op.startswith("v_mul_f32"):
            R[args[0]] = mul(val(args[1]), val(args[2]))
        elif op.startswith("v_fma_f32"):
            R[args[0]] = fma(val(args[1]), val(args[2]), val(args[3]))
        elif op.startswith("v_fmac_f32"):
            R[args[0]] = fma(val(args[1]), val(args[2]), val(args[0]))
        elif op in ("v_pk_mul_f32", "v_pk_fma_f32"):
            n = 2 if op == "v_pk_mul_f32" else 3
            src = [regs(a) for a in args[1:1 + n]]
            sel, selh = md.get("op_sel", [0] * n), md.get("op_sel_hi", [1] * n)
            ngl, ngh = md.get("neg_lo", [0] * n), md.get("neg_hi", [0] * n)
            res = []
            for half, (ss, ng) in enumerate(((sel, ngl), (selh, ngh))):
                v = []
                for k in range(n):
                    r = src[k]
                    e = val(r[ss[k]] if len(r) == 2 else r[0])     # (a 32-bit constant feeds both halves)
                    v.append(neg(e) if ng[k] else e)
                res.append(mul(*v) if n == 2 else fma(*v))
            d = regs(args[0])
            R[d[0]], R[d[1]] = res
        elif op == "v_pk_add_f32" and args[2] == "0" and md.get("neg_lo") == [1, 1] and md.get("neg_hi") == [1, 1]:
            d, s2 = regs(args[0]), regs(args[1])     # -x + -0 = -x exactly: the compiler's packed negation
            sel, selh = md.get("op_sel", [0, 0]), md.get("op_sel_hi", [1, 1])
            vals = [neg(val(s2[sel[0]])), neg(val(s2[selh[0]]))]
            R[d[0]], R[d[1]] = vals
        elif op.startswith(("v_sin_f32", "v_cos_f32")):
            R[args[0]] = S.node(op[2:5], val(args[1]))
        elif op.startswith("v_mov_b32") and "dpp" not in op:
            R[args[0]] = val(args[1])
            if lit(args[1]) is not None and 0x1000 <= lit(args[1]) < 0x28000:
                base[args[0]] = lit(args[1])
            elif args[1] in base:
                base[args[0]] = base[args[1]]
        elif op.startswith("v_mov_b64"):
            d, s = regs(args[0]), regs(args[1])
            vals = [val(s[k] if len(s) == 2 else s[0]) for k in range(2)]
            R[d[0]], R[d[1]] = vals
        elif op == "v_pk_mov_b32":
            d, a, b = regs(args[0]), regs(args[1]), regs(args[2])
            sel = md.get("op_sel", [0, 1])
            vals = [val(a[sel[0]]), val(b[sel[1]])]
            R[d[0]], R[d[1]] = vals
        elif op.startswith("v_cndmask_b32"):
            R[args[0]] = S.node("sel", val(args[1]), val(args[2]))
            bs = [base[x] for x in args[1:3] if x in base] + [v for v in map(lit, args[1:3]) if v is not None and 0x1000 <= v < 0x28000]
            base.pop(args[0], None)
            if bs:
                base[args[0]] = max(bs)
        elif op.startswith("v_xor_b32") and "0x80000000" in args[1:]:
            o = args[2] if args[1] == "0x80000000" else args[1]
            R[args[0]] = neg(val(o))
        elif op == "ds_bpermute_b32":
            R[args[0]] = S.node("shfl", val(args[2]))
        elif op.startswith("ds_read"):
            d = regs(args[0])
            loads.append((base.get(args[1], 0) + off, d, len(S.text)))
            for k, r in enumerate(d):
                R[r] = "LD%d.%d" % (len(loads) - 1, k)
        elif op.startswith(("global_load", "buffer_load", "flat_load")):
            for k, r in enumerate(regs(args[0])):
                R[r] = "G.%d" % k
        elif op.startswith("ds_write"):
            for r in regs(args[1]):
                e = R.get(r)
                if e is not None and S.fp(e) and record:
                    outs.append(("lds", e))
        elif op.startswith("v_cvt_pk_") and op.endswith("_f32"):
            for a in args[1:3]:
                if record:
                    outs.append(("cvt", val(a)))
            R[args[0]] = "packed"
        elif op.startswith("v_") and args:
            # integer / address arithmetic: the result carries the largest LDS base among its operands
            b = [base[a] for a in args[1:] if a in base] + [v for v in (lit(a) for a in args[1:]) if v is not None and 0x1000 <= v < 0x28000]
            for r in regs(args[0]):
                R[r] = "I"
                base.pop(r, None)
                if b and re.match(r"v_(add|lshl_add|lshl_or|or|and_or|or3|add_lshl|mad_u32|bitop3|xad|cndmask)", op):
                    base[r] = max(b)

    mfma0 = next((i for i, l in enumerate(body) if "v_mfma" in l), len(body))
    seen_line = set()

    def run():
        nonlocal R, base
        for i in range(mfma0):
            l = body[i]
            m = re.match(r"^\s+s_cbranch_\w+ (\.LBB\d+_\d+)", l)
            tgt = label_at.get(m.group(1), -1) if m else -1
            if tgt > mfma0 and tgt not in seen_line:
                # predicated regions the compiler moved behind the kernel's main path (they branch back into it):
                # evaluated from the state at the branch, which the main path then continues from
                keep = (dict(R), dict(base))
                k = tgt
                while k < len(body) and "v_mfma" not in body[k] and not re.match(r"^\s+s_branch ", body[k]):
                    step(body[k], k)
                    k += 1
                R, base = keep
            step(l, i)

    run()
    # name the LDS arrays by rank of their base address (a base inside the previous array's bytes belongs to it)
    used, todo = set(), [e for _, e in outs]
    while todo:
        h = todo.pop()
        if h in used:
            continue
        used.add(h)
        if h in S.text:
            todo += list(S.text[h][1])
    bases = sorted({b for i, (b, d, _) in enumerate(loads) if any("LD%d.%d" % (i, k) in used for k in range(len(d)))})
    rank, groups = {}, []
    for b in bases:
        if not groups or b - groups[-1] >= GEN_ARRAYS[min(len(groups), len(GEN_ARRAYS)) - 1]:
            groups.append(b)
        rank[b] = len(groups) - 1
    ren = {}
    for i, (b, d, _) in enumerate(loads):
        for k in range(len(d)):
            if b not in rank:
                continue
            r = rank[b] if perm is None else perm[rank[b]]
            ren["LD%d.%d" % (i, k)] = "lds%d.%s" % (r, "xyzw"[k] if len(d) > 1 else "s")

    memo, dmemo = {}, {}

    def depth(h):
        if h not in dmemo:
            dmemo[h] = 1 + max(depth(k) for k in C.text[h][1]) if h in C.text else 0
        return dmemo[h]

    def canon(h):
        if h in memo:
            return memo[h]
        if h in ren:
            r = ren[h]
        elif h not in S.text:
            r = h
        else:
            op, kids = S.text[h]
            ck = [canon(k) for k in kids]
            if op == "mul":
                ck = sorted(ck)
            elif op in ("fma", "fnma"):
                ck = sorted(ck[:2]) + ck[2:]
            prod = sorted((k for k in ck if k in C.text and C.text[k][0] in ("mul", "fma", "fnma")), key=depth)
            r = prod[-1] if taken and op == "sel" and prod else C.node(op, *ck)
        memo[h] = r
        return r

    C = Sym()
    res = sorted((kind, canon(e)) for kind, e in outs if kind == "cvt" or S.fp(e))
    if os.environ.get('HEA_GEN_ISA_DEBUG'):
        print('  bases', [hex(b) for b in bases], 'arrays', [hex(g) for g in groups])
    return res, C, counts, len(groups)


DESC_KEYS = ["float_round_mode_32", "float_round_mode_16_64", "float_denorm_mode_32", "float_denorm_mode_16_64", "ieee_mode",
             "dx10_clamp", "NumVgprs", "NumAgprs", "TotalNumSgprs", "group_segment_fixed_size", "private_segment_fixed_size",
             "ScratchSize", "Occupancy"]
MODE_KEYS = DESC_KEYS[:6]


def report(name, body, desc, verbose=True):
    res, C, counts, _ = evaluate(body)
    print("kernel", name)
    print("  descriptor:", ", ".join(f"{k}={desc.get(k, '-')}" for k in DESC_KEYS))
    print("  fp instructions up to the first MFMA:", ", ".join(f"{k} x{v}" for k, v in sorted(counts.items())))
    digest = hashlib.sha1(repr(res).encode()).hexdigest()[:16]
    print(f"  values leaving the block: {len(res)}  (digest {digest})")
    if verbose:
        seen = {}
        for kind, h in res:
            seen[(kind, h)] = seen.get((kind, h), 0) + 1
        for (kind, h), n in sorted(seen.items()):
            print(f"    {kind} x{n:<3d} {h}  {C.show(h, 3)}")
    return res, desc


def cmd_asm(src, out, extra):
    inc = ["-I", os.path.dirname(os.path.abspath(src))] + extra
    subprocess.run(["hipcc", *FLAGS, *inc, "-x", "hip", src, "-o", out], check=True)


def cmd_spec(out, retile=None):
    sys.path.insert(0, ROOT)
    from qfedx_amd.models.vqc import VQCSpec
    from qfedx_amd.ops._ext import ext
    from qfedx_amd.ops.hea_mfma import HeaMfmaProgram
    prog = HeaMfmaProgram(VQCSpec(n_qubits=16, n_layers=3, n_classes=3), "cpu", use_spec=False,
                          **({"tile_bits": retile, "adj_tile_bits": retile} if retile else {}))
    (f, ff), _ = prog._host_progs[0]
    open(out, "w").write(ext().hea_spec_source(False, f, ff, prog.spec_cfg(0, False)))


def compare(na, ra, da, nb, rb, db, sub=None):
    """``sub``: the first kernel's expressions.  A value only the second kernel stores is accepted when the first
    computes it on the way to a value it stores: a half table of fewer factors than the interpreter's predicated chain
    of seven (tiles below 2^14), which the per-plan kernel ends at the plan's count."""
    ok = ra == rb
    if not ok and sub is not None and not set(ra) - set(rb) and all(h in sub.text for _, h in set(rb) - set(ra)):
        print("   (the second kernel also stores", len(set(rb) - set(ra)), "value(s) the first computes inside a longer chain)")
        ok = True
    modes = all(da.get(k) == db.get(k) for k in MODE_KEYS)
    print(f"{'SAME' if ok else 'DIFFERENT'} values, float modes {'equal' if modes else 'DIFFER'}: {na}  |  {nb}")
    if not ok:
        a, b = set(ra), set(rb)
        print("   only in first :", sorted(a - b)[:8])
        print("   only in second:", sorted(b - a)[:8])
    return ok and modes


def main():
    a = sys.argv[1:]
    if a[0] == "asm":
        cmd_asm(a[1], a[2], a[3:])
    elif a[0] == "spec":
        cmd_spec(a[1], int(a[3]) if len(a) > 3 and a[2] == "--retile" else None)
    elif a[0] == "show":
        for name, (body, desc) in kernels(a[1]).items():
            if len(a) < 3 or a[2] in name:
                report(name, body, desc)
    elif a[0] == "diff":
        ka, kb = kernels(a[1]), kernels(a[2])
        bad = 0
        for name in ka:
            ra = evaluate(ka[name][0])[0]
            rb = evaluate(kb[name][0])[0]
            bad += not compare(a[1] + ":" + name, ra, ka[name][1], a[2] + ":" + name, rb, kb[name][1])
        sys.exit(1 if bad else 0)
    elif a[0] == "same":
        (na, (ba, da)), = [(n, v) for n, v in kernels(a[1]).items() if a[2] in n]
        (nb, (bb, db)), = [(n, v) for n, v in kernels(a[3]).items() if a[4] in n]
        # the two builds lay LDS out differently: equal under SOME renaming of the arrays the block reads
        import itertools
        ra, Ca, _, n = evaluate(ba, taken=True)
        rbs = [evaluate(bb, perm=pm, taken=True)[0] for pm in itertools.permutations(range(max(n, evaluate(bb)[3])))]
        rb = next((r for r in rbs if r == ra), rbs[0])
        sys.exit(0 if compare(na, ra, da, nb, rb, db, Ca) else 1)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
