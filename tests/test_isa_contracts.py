"""CPU: the edge scorer's inline-assembly contracts, checked in the gfx950 ISA of the library the build produced.

hipcc treats an `asm` statement as one opaque instruction: it neither pads the hazards of the instructions inside nor counts their
memory operations (cdna_hip_programming.md-style rules, see csrc/edge_score.hip at shift_in_bit and dma_one).  Four facts keep the
scorer correct and only the compiler's output can confirm them, so this module disassembles every code object of libsgs_hip.so and
checks them in every kernel that contains the assembly:

R1  mask hazard: a v_addc_co_u32_e64 whose carry-in SGPR pair was last written by a VALU instruction has >= 2 wait states after it.
R2  M0: in a kernel with an LDS-DMA (global_load_lds*) the only instructions that name or implicitly read M0 are the DMA statement's
    `s_mov_b32 m0, sX` / `s_nop 0` / load triple.
R3  SGPR base: an SGPR that an asm VMEM instruction (the LDS-DMA) reads was not written by a VALU fewer than 5 wait states earlier.
R4  counted waits: after an LDS-DMA, the first s_waitcnt that bounds vmcnt (vmcnt(N)) has >= N VMEM instructions issued between the
    DMA and itself (so it retires the DMA), and an s_barrier follows it before the next ds_read.

Every scan follows the control flow: a backward scan that reaches the start of a basic block continues into EVERY predecessor, a
forward scan into every successor; an unresolvable branch fails the check.  Per-family minimum site counts keep the checks from
passing on an empty listing, and hand-written listings that break each rule (negative controls) must be rejected.
"""
import os
import re
import subprocess
from collections import defaultdict

import pytest

BUNDLER = "/opt/rocm/lib/llvm/bin/clang-offload-bundler"
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


# ----------------------------------------------------------------------------------------------------------------------------------
# listing -> per-kernel instruction streams and basic blocks

_FUNC = re.compile(r"^([0-9a-fA-F]+) <([^>]+)>:\s*$")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)(?:\s+(.*?))?\s*//\s*([0-9A-Fa-f]+):")
_TARGET = re.compile(r"<([^>+]+)\+0x([0-9a-fA-F]+)>\s*$")


class Insn:
    __slots__ = ("op", "args", "addr", "target", "ops")

    def __init__(self, op, args, addr, target):
        self.op, self.args, self.addr, self.target = op, args, addr, target
        self.ops = [x.strip() for x in _split_operands(args)]

    def __repr__(self):
        return f"{self.addr:#x}: {self.op} {self.args}"


def _split_operands(args):
    out, depth, cur = [], 0, ""
    for ch in args:
        if ch in "[(":
            depth += 1
        elif ch in "])":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return out                       # (modifiers such as offset:16 stay inside the last operand, after a blank: sregs() reads the first word)


def parse_listing(text):
    """llvm-objdump -d text -> {kernel name: [Insn]} in address order."""
    funcs, cur, base = {}, None, 0
    for line in text.splitlines():
        m = _FUNC.match(line)
        if m:
            cur, base = m.group(2), int(m.group(1), 16)
            funcs[cur] = []
            continue
        if cur is None:
            continue
        m = _INSN.match(line)
        if not m:
            continue
        op, args, addr = m.group(1), (m.group(2) or "").strip(), int(m.group(3), 16)
        target = None
        t = _TARGET.search(line)
        if op.startswith(("s_branch", "s_cbranch")):
            if not t or t.group(1) != cur:
                raise AssertionError(f"{cur}: branch without a resolvable in-function target: {line.strip()}")
            target = base + int(t.group(2), 16)
        funcs[cur].append(Insn(op, args, addr, target))
    return funcs


class CFG:
    """Basic blocks of one kernel: leaders at branch targets and after every branch / s_endpgm."""

    def __init__(self, name, insns):
        self.name, self.insns = name, insns
        by_addr = {x.addr: i for i, x in enumerate(insns)}
        for x in insns:
            if x.op.startswith(("s_setpc", "s_swappc", "s_cbranch_g_fork", "s_cbranch_join")):
                raise AssertionError(f"{name}: indirect control flow at {x!r}: the scans cannot follow it")
        leaders = {0}
        for i, x in enumerate(insns):
            if x.target is not None:
                if x.target not in by_addr:
                    raise AssertionError(f"{name}: branch at {x!r} targets {x.target:#x}, not an instruction of the kernel")
                leaders.add(by_addr[x.target])
            if x.target is not None or x.op == "s_endpgm":
                if i + 1 < len(insns):
                    leaders.add(i + 1)
        starts = sorted(leaders)
        self.block_of = [0] * len(insns)
        self.blocks = []                    # (first, last) instruction indices
        for b, s in enumerate(starts):
            e = (starts[b + 1] if b + 1 < len(starts) else len(insns)) - 1
            self.blocks.append((s, e))
            for i in range(s, e + 1):
                self.block_of[i] = b
        self.succ = [[] for _ in self.blocks]
        self.pred = [[] for _ in self.blocks]
        for b, (s, e) in enumerate(self.blocks):
            last = insns[e]
            outs = []
            if last.target is not None:
                outs.append(self.block_of[by_addr[last.target]])
            falls = last.op != "s_endpgm" and last.op != "s_branch"
            if falls and b + 1 < len(self.blocks):
                outs.append(b + 1)
            for o in outs:
                self.succ[b].append(o)
                self.pred[o].append(b)


# ----------------------------------------------------------------------------------------------------------------------------------
# operand classes

_SREG = re.compile(r"^s\[(\d+):(\d+)\]$|^s(\d+)$|^(vcc|exec|flat_scratch|xnack_mask)(_lo|_hi)?$|^(m0)$")


def sregs(operand):
    """The scalar registers an operand names (empty for VGPRs, literals, modifiers)."""
    tok = operand.split()[0] if operand else ""
    tok = tok.lstrip("-!|").rstrip("|")
    m = _SREG.match(tok)
    if not m:
        return set()
    if m.group(1) is not None:
        return {f"s{i}" for i in range(int(m.group(1)), int(m.group(2)) + 1)}
    if m.group(3) is not None:
        return {f"s{m.group(3)}"}
    if m.group(6):
        return {"m0"}
    base, half = m.group(4), m.group(5)
    return {base + half} if half else {base + "_lo", base + "_hi"}


_SALU_NO_DST = ("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_nop", "s_waitcnt", "s_barrier", "s_setprio", "s_sleep", "s_endpgm",
                "s_store", "s_buffer_store", "s_sendmsg", "s_trap", "s_dcache", "s_setreg", "s_ttracedata", "s_icache", "s_set_gpr_idx",
                "s_sethalt", "s_setkill", "s_incperflevel", "s_decperflevel", "s_scratch_store")
_VOP3B = ("v_add_co_u32_e64", "v_sub_co_u32_e64", "v_subrev_co_u32_e64", "v_addc_co_u32_e64", "v_subb_co_u32_e64",
          "v_subbrev_co_u32_e64", "v_div_scale_f32", "v_div_scale_f64", "v_mad_u64_u32", "v_mad_i64_i32")


def is_valu(x):
    return x.op.startswith("v_")


def sgpr_writes(x):
    """Scalar registers the instruction writes (explicit destinations and the implicit VCC / EXEC of VOPC and carry forms)."""
    op, ops = x.op, x.ops
    if op.startswith("v_"):
        w = set()
        if ops:
            w |= sregs(ops[0])                                      # v_cmp*_e64 sdst, v_readlane / v_readfirstlane dst
        if op.startswith(_VOP3B) and len(ops) > 1:
            w |= sregs(ops[1])                                      # carry-out / VCC-out of the VOP3b forms
        if op.endswith("_e32") and (op.startswith("v_cmp") or "_co_" in op or op.startswith(("v_addc", "v_subb"))):
            w |= {"vcc_lo", "vcc_hi"}
        if op.startswith("v_cmpx"):
            w |= {"exec_lo", "exec_hi"}
        return w
    if op.startswith("s_"):
        if op.startswith(_SALU_NO_DST) or not ops:
            return set()
        return sregs(ops[0])
    return set()


def sgpr_reads_of_vmem(x):
    """Scalar operands of a vector-memory instruction (base address pair, soffset, descriptor)."""
    r = set()
    for o in x.ops[1:]:
        r |= sregs(o)
    return r - {"m0"}


def is_vmem(x):
    return x.op.startswith(("global_", "buffer_", "flat_", "scratch_", "tbuffer_"))


def is_dma(x):
    return x.op.startswith("global_load_lds") or (x.op.startswith("buffer_load") and re.search(r"\blds\b", x.args) is not None)


def wait_states(x):
    if x.op == "s_nop":
        return int(x.ops[0], 0) + 1 if x.ops else 1
    return 1


def vmcnt_of(x):
    if x.op != "s_waitcnt":
        return None
    m = re.search(r"vmcnt\((\d+)\)", x.args)
    return int(m.group(1)) if m else None


# ----------------------------------------------------------------------------------------------------------------------------------
# scans

def _backward_hazard(cfg, i, regs, need):
    """Distances (wait states) from every VALU writer of `regs` that reaches instruction i within fewer than `need` wait states, over all
    paths.  Returns the list of offending (writer, wait states) pairs; a non-VALU writer ends a path harmlessly."""
    bad, seen = [], set()
    stack = [(cfg.block_of[i], i - 1, 0, frozenset(regs))]
    while stack:
        b, j, ws, left = stack.pop()
        s, _ = cfg.blocks[b]
        while j >= s and left and ws < need:
            x = cfg.insns[j]
            hit = sgpr_writes(x) & left
            if hit:
                if is_valu(x):
                    bad.append((x, ws))
                left = left - hit                               # each register's search ends at its last writer
            ws += wait_states(x)
            j -= 1
        if not left or ws >= need:
            continue
        for p in cfg.pred[b]:
            key = (p, ws, left)
            if key not in seen:
                seen.add(key)
                stack.append((p, cfg.blocks[p][1], ws, left))
    return bad


def check_r1(cfg):
    """v_addc_co_u32_e64: carry-in (last operand) after a VALU write of that pair needs 2 wait states."""
    sites, errs = 0, []
    for i, x in enumerate(cfg.insns):
        if x.op != "v_addc_co_u32_e64":
            continue
        sites += 1
        cin = sregs(x.ops[-1])
        for w, ws in _backward_hazard(cfg, i, cin, 2):
            errs.append(f"R1 {cfg.name}: {x!r} reads {x.ops[-1]} {ws} wait state(s) after VALU {w!r}")
    return sites, errs


_M0_IMPLICIT = ("s_sendmsg", "s_ttracedata", "ds_gws", "ds_append", "ds_consume", "ds_ordered_count", "s_movrel", "v_movrel", "v_interp",
                "s_set_gpr_idx")


def _names_m0(x):
    return any("m0" in sregs(o) for o in x.ops) or re.search(r"\bm0\b", x.args) is not None


def check_r2(cfg):
    """In a kernel with an LDS-DMA, M0 belongs to the DMA statements alone."""
    insns = cfg.insns
    dmas = [i for i, x in enumerate(insns) if is_dma(x)]
    if not dmas:
        return 0, []
    errs, owned = [], set()
    for i in dmas:
        ok = (i >= 2 and insns[i - 1].op == "s_nop" and insns[i - 1].ops == ["0"] and insns[i - 2].op == "s_mov_b32"
              and insns[i - 2].ops[:1] == ["m0"] and cfg.block_of[i - 2] == cfg.block_of[i])
        if not ok:
            errs.append(f"R2 {cfg.name}: {insns[i]!r} is not preceded by its own `s_mov_b32 m0, sX` and `s_nop 0`")
        else:
            owned.add(i - 2)
    for i, x in enumerate(insns):
        if i in owned or is_dma(x):
            continue
        implicit = x.op.startswith(_M0_IMPLICIT) or "addtid" in x.op or (x.op.endswith("_lds") or "_lds_" in x.op)
        if implicit or _names_m0(x):
            errs.append(f"R2 {cfg.name}: {x!r} uses M0 in a kernel whose LDS-DMA statements own it")
    return len(dmas), errs


def check_r3(cfg):
    """The asm VMEM instructions (the LDS-DMAs): SGPR operands not written by a VALU fewer than 5 wait states earlier."""
    sites, errs = 0, []
    for i, x in enumerate(cfg.insns):
        if not is_dma(x):
            continue
        sites += 1
        for w, ws in _backward_hazard(cfg, i, sgpr_reads_of_vmem(x), 5):
            errs.append(f"R3 {cfg.name}: {x!r} reads an SGPR {ws} wait state(s) after VALU {w!r}")
    return sites, errs


def check_r4(cfg):
    """Every LDS-DMA: along every path, the first vmcnt-bounding wait retires it (>= N VMEM issued since), and an s_barrier comes
    after that wait before any ds_read.  Returns (DMA count, {N: count of counted waits that retire a DMA}, errors)."""
    insns, errs, waits = cfg.insns, [], defaultdict(set)
    n_dma = 0
    for i, x in enumerate(insns):
        if not is_dma(x):
            continue
        n_dma += 1
        # state: (block, index, VMEM issued since the DMA, retired?)
        stack, seen = [(cfg.block_of[i], i + 1, 0, False)], set()
        while stack:
            b, j, vm, retired = stack.pop()
            _, e = cfg.blocks[b]
            end = False
            while j <= e:
                y = insns[j]
                n = vmcnt_of(y)
                if not retired:
                    if n is not None:
                        if n > vm:
                            errs.append(f"R4 {cfg.name}: {y!r} after {x!r} with only {vm} VMEM instruction(s) between: the DMA is not retired")
                            end = True
                            break
                        retired = True
                        waits[n].add(j)
                    elif y.op == "s_barrier":
                        errs.append(f"R4 {cfg.name}: {y!r} reached from {x!r} before any vmcnt wait")
                        end = True
                        break
                    elif y.op == "s_endpgm":
                        errs.append(f"R4 {cfg.name}: {y!r} reached from {x!r} with the DMA never waited for")
                        end = True
                        break
                    elif is_vmem(y):
                        vm += 1
                else:
                    if y.op == "s_barrier":
                        end = True
                        break
                    if y.op.startswith("ds_read") or y.op == "s_endpgm":
                        errs.append(f"R4 {cfg.name}: {y!r} after the wait retiring {x!r} but before any s_barrier")
                        end = True
                        break
                j += 1
            if end:
                continue
            for s_ in cfg.succ[b]:
                key = (s_, min(vm, 64), retired)
                if key not in seen:
                    seen.add(key)
                    stack.append((s_, cfg.blocks[s_][0], vm, retired))
    return n_dma, {n: len(v) for n, v in waits.items()}, errs


def check_kernel(name, insns):
    cfg = CFG(name, insns)
    r1_sites, e1 = check_r1(cfg)
    r2_sites, e2 = check_r2(cfg)
    r3_sites, e3 = check_r3(cfg)
    n_dma, waits, e4 = check_r4(cfg)
    return {"addc": r1_sites, "dma": n_dma, "waits": waits, "errors": e1 + e2 + e3 + e4}


def check_listing(text):
    return {name: check_kernel(name, insns) for name, insns in parse_listing(text).items()}


# ----------------------------------------------------------------------------------------------------------------------------------
# the library's listing

def _disassemble(lib_path, tmp):
    """Every gfx950 code object of the library (one bundle per translation unit in .hip_fatbin), disassembled into one text."""
    sect = os.path.join(tmp, "fatbin.bin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib_path, sect], check=True)
    blob = open(sect, "rb").read()
    offs = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), blob)]
    assert offs, "no offload bundle in the library's .hip_fatbin section"
    texts = []
    for k, o in enumerate(offs):
        end = offs[k + 1] if k + 1 < len(offs) else len(blob)
        bpath, cpath = os.path.join(tmp, f"b{k}.bin"), os.path.join(tmp, f"c{k}.co")
        with open(bpath, "wb") as f:
            f.write(blob[o:end])
        subprocess.run([BUNDLER, "--unbundle", "--type=o", f"--input={bpath}", f"--targets={TARGET}", f"--output={cpath}"], check=True)
        r = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", cpath], capture_output=True, text=True, check=True)
        texts.append(r.stdout)
    return "\n".join(texts)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    import __graft_entry__ as ge
    ge.build()
    import sgs_gnn_amd
    for tool in (BUNDLER, OBJDUMP):
        assert os.path.exists(tool), f"{tool} missing: the ISA contracts cannot be checked"
    text = _disassemble(sgs_gnn_amd._lib.LIB_PATH, str(tmp_path_factory.mktemp("isa")))
    return check_listing(text)


_BF16X6 = re.compile(r"edge_score_bf16x6_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE")


def _bf16x6(results):
    out = {}
    for name, r in results.items():
        m = _BF16X6.search(name)
        if m:
            out[tuple(int(g) for g in m.groups())] = r           # (NT, NW, MODE, NP)
    return out


def test_every_kernel_satisfies_the_contracts(results):
    errors = [e for r in results.values() for e in r["errors"]]
    assert not errors, f"{len(errors)} contract violation(s):\n" + "\n".join(errors[:40])


def test_every_scorer_instantiation_is_present(results):
    k = _bf16x6(results)
    want = {(nt, 4, mode, 3) for nt in (4, 8) for mode in (0, 1, 2, 3, 4, 5)} | {(nt, 4, mode, 1) for nt in (4, 8) for mode in (0, 3, 4, 5)}
    assert want <= set(k), f"edge_score_bf16x6_kernel instantiations missing from the listing: {sorted(want - set(k))}"


def test_mask_keeping_forwards_have_every_carry_in_site(results):
    """MODEs 0 / 3 run shift_in_bit once per hidden unit and direction in each of the two mask-keeping epilogues (dropout on / off)."""
    for (nt, nw, mode, np_), r in _bf16x6(results).items():
        if mode not in (0, 3):
            continue
        need = 2 * 16 * nt * (2 if mode == 3 else 1)          # (4 NT steps x 4 units) x 2 epilogues x directions
        assert r["addc"] >= need, f"bf16x6<{nt},{nw},{mode},{np_}>: {r['addc']} v_addc_co_u32_e64 sites, expected >= {need}"


def test_every_bf16x6_instantiation_has_its_dmas(results):
    """dma_one runs SPT = NT NP / 4 times in the prologue and in each of the two phases of the loop body."""
    for (nt, nw, mode, np_), r in _bf16x6(results).items():
        spt = nt * np_ * 64 // (64 * nw)
        assert r["dma"] >= 3 * spt, f"bf16x6<{nt},{nw},{mode},{np_}>: {r['dma']} LDS-DMAs, expected >= {3 * spt}"


def test_one_piece_instantiations_have_their_counted_waits(results):
    """The one-piece phase retires its DMA with vmcnt(kFL): kFL = 4 feature loads (MODEs 0, 3), 1 mask byte (MODEs 4, 5)."""
    for (nt, nw, mode, np_), r in _bf16x6(results).items():
        if np_ != 1:
            continue
        n = 1 if mode in (4, 5) else 4
        assert r["waits"].get(n, 0) >= 2, f"bf16x6<{nt},{nw},{mode},1>: {r['waits']} DMA-retiring waits, expected two vmcnt({n})"


# ----------------------------------------------------------------------------------------------------------------------------------
# negative controls: each breaks one rule, the checker must say so

def _listing(name, lines):
    out, addr = [f"0000000000001000 <{name}>:"], 0x1000
    for ln in lines:
        if ln.endswith(":"):                                   # a label: resolved below
            out.append(ln)
            continue
        out.append(f"\t{ln:<58}// {addr:012X}: 00000000")
        addr += 4
    # labels -> branch targets of the form <name+0xOFF>
    labels, addr, body = {}, 0x1000, []
    for ln in out[1:]:
        if ln.endswith(":"):
            labels[ln[:-1]] = addr
        else:
            body.append(ln)
            addr += 4
    res = [out[0]]
    for ln in body:
        m = re.search(r"@(\w+)", ln)
        if m:
            ln = ln.replace("@" + m.group(1), "1") + f" <{name}+{labels[m.group(1)] - 0x1000:#x}>"
        res.append(ln)
    return "\n".join(res) + "\n"


def _errors(text, rule):
    return [e for r in check_listing(text).values() for e in r["errors"] if e.startswith(rule)]


def test_control_r1_unpadded_compare_mask_is_rejected():
    ok = _listing("k", ["v_cmp_lt_f32_e64 s[0:1], 0, v1", "s_nop 1", "v_addc_co_u32_e64 v2, s[0:1], v2, v2, s[0:1]", "s_endpgm"])
    bad = _listing("k", ["v_cmp_lt_f32_e64 s[0:1], 0, v1", "v_addc_co_u32_e64 v2, s[0:1], v2, v2, s[0:1]", "s_endpgm"])
    salu = _listing("k", ["v_cmp_lt_f32_e64 s[2:3], 0, v1", "s_and_b64 s[0:1], s[2:3], s[4:5]",
                          "v_addc_co_u32_e64 v2, s[0:1], v2, v2, s[0:1]", "s_endpgm"])
    one = _listing("k", ["v_cmp_lt_f32_e64 s[0:1], 0, v1", "v_mov_b32_e32 v3, 0", "v_addc_co_u32_e64 v2, s[0:1], v2, v2, s[0:1]", "s_endpgm"])
    assert not _errors(ok, "R1") and not _errors(salu, "R1")
    assert _errors(bad, "R1") and _errors(one, "R1")


def test_control_r1_follows_every_predecessor():
    """The padded fall-through path is fine; the branch path brings the compare's result unpadded."""
    text = _listing("k", ["s_cmp_eq_u32 s4, 0", "v_cmp_lt_f32_e64 s[0:1], 0, v1", "s_cbranch_scc1 @join", "s_nop 4", "join:",
                          "v_addc_co_u32_e64 v2, s[0:1], v2, v2, s[0:1]", "s_endpgm"])
    assert _errors(text, "R1")


def _dma(sreg="s6", base="s[8:9]"):
    return [f"s_mov_b32 m0, {sreg}", "s_nop 0", f"global_load_lds_dwordx4 v0, {base}"]


def test_control_r2_foreign_m0_use_is_rejected():
    ok = _listing("k", _dma() + ["s_waitcnt vmcnt(0)", "s_barrier", "ds_read_b128 v[4:7], v1", "s_endpgm"])
    reader = _listing("k", ["s_mov_b32 m0, s7", "s_sendmsg sendmsg(MSG_INTERRUPT)"] + _dma()
                      + ["s_waitcnt vmcnt(0)", "s_barrier", "s_endpgm"])
    named = _listing("k", _dma() + ["v_readlane_b32 s10, v3, m0", "s_waitcnt vmcnt(0)", "s_barrier", "s_endpgm"])
    no_nop = _listing("k", ["s_mov_b32 m0, s6", "global_load_lds_dwordx4 v0, s[8:9]", "s_waitcnt vmcnt(0)", "s_barrier", "s_endpgm"])
    assert not _errors(ok, "R2")
    assert _errors(reader, "R2") and _errors(named, "R2") and _errors(no_nop, "R2")


def test_control_r3_fresh_valu_base_is_rejected():
    bad = _listing("k", ["v_readfirstlane_b32 s8, v5", "s_mov_b32 s9, 0"] + _dma() + ["s_waitcnt vmcnt(0)", "s_barrier", "s_endpgm"])
    ok = _listing("k", ["v_readfirstlane_b32 s8, v5", "s_nop 4"] + _dma() + ["s_waitcnt vmcnt(0)", "s_barrier", "s_endpgm"])
    assert _errors(bad, "R3") and not _errors(ok, "R3")


def test_control_r4_short_count_and_early_read_are_rejected():
    loads = ["global_load_dwordx4 v[10:13], v[20:21], off"] * 4
    ok = _listing("k", _dma() + loads + ["s_waitcnt vmcnt(4)", "s_barrier", "ds_read_b128 v[4:7], v1", "s_endpgm"])
    short = _listing("k", _dma() + loads + ["s_waitcnt vmcnt(5)", "s_barrier", "ds_read_b128 v[4:7], v1", "s_endpgm"])
    early = _listing("k", _dma() + loads + ["s_waitcnt vmcnt(4)", "ds_read_b128 v[4:7], v1", "s_barrier", "s_endpgm"])
    nowait = _listing("k", _dma() + loads + ["s_barrier", "s_waitcnt vmcnt(0)", "s_endpgm"])
    assert not _errors(ok, "R4")
    assert _errors(short, "R4") and _errors(early, "R4") and _errors(nowait, "R4")


def test_control_r4_follows_every_successor():
    """One successor waits correctly, the other reaches the barrier with a count that does not cover the DMA."""
    text = _listing("k", _dma() + ["global_load_dwordx4 v[10:13], v[20:21], off", "s_cbranch_scc1 @other", "s_waitcnt vmcnt(1)",
                                   "s_branch @join", "other:", "s_waitcnt vmcnt(2)", "join:", "s_barrier", "s_endpgm"])
    assert _errors(text, "R4")


def test_control_unresolvable_branch_fails_loudly():
    text = "0000000000001000 <k>:\n\ts_cbranch_scc1 3   // 000000001000: BF850003 <other+0x10>\n\ts_endpgm   // 000000001004: BF810000\n"
    with pytest.raises(AssertionError, match="resolvable"):
        check_listing(text)
