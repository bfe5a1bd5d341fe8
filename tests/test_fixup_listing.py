"""CPU tier: what the compiler made of the WBFM boundary fix-up's trips to memory (iqd_stream_fix.h: wbfm_stream_fixup_body).

The source has asked for "everything at once" since round 2, and the generated gfx950 code did not do it: it waited for the
segment's channel before anything else and staged the boundary records in a loop of single dwords with a wait in every turn -
six dependent trips per workgroup in a kernel that is nothing but its trips.  This compiles iqd_stream.hip the way
tools/isa_lint.py does and holds the stretch of wbfm_stream_fixup_kernel in front of its first barrier to: no loop, the
records as 16-byte loads and no single dword of them, and two waits for memory at the most on the way of a launch that is not
squelch-gated."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN3iqd24wbfm_stream_fixup_kernelENS_11ChainLaunchENS_10StreamArgsE"
REG = re.compile(r"\b([sv])\[(\d+):(\d+)\]|\b([sv])(\d+)\b")


def regs_of(text):
    out = set()
    for m in REG.finditer(text):
        if m.group(4) is not None:
            out.add((m.group(4), int(m.group(5))))
        else:
            out.update((m.group(1), k) for k in range(int(m.group(2)), int(m.group(3)) + 1))
    return out


@pytest.fixture(scope="module")
def listing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    return isa_lint.compile_to_asm(os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_stream.hip"))


def hist_kernarg_offset(text):
    """StreamArgs is the kernel's second argument and `hist` its first member: the second .offset of the kernel's metadata."""
    meta = text[text.index("amdhsa.kernels"):]
    args = meta[:re.search(r"\.name:\s+" + KERNEL + r"\s*\n", meta).start()]
    args = args[args.rindex(".args:"):]
    offsets = [int(v) for v in re.findall(r"\.offset:\s+(\d+)", args)]
    sizes = [int(v) for v in re.findall(r"\.size:\s+(\d+)", args)]
    assert len(offsets) >= 2 and offsets[0] == 0 and sizes[0] <= offsets[1], (offsets, sizes)
    return offsets[1]


def front_stretch(text):
    """[(op, operands, line)] from the kernel's start to its first s_barrier, labels as ("label", name, line)"""
    body = text[text.index("\n" + KERNEL + ":"):]
    out = []
    for raw in body.splitlines()[2:]:
        line = raw.strip()
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            out.append(("label", m.group(1), line))
            continue
        if not line or line[0] in ";.":
            continue
        code = line.partition(";")[0].strip()
        op, _, rest = code.partition(" ")
        out.append((op, [o.strip() for o in rest.split(",")] if rest.strip() else [], line))
        if op == "s_barrier":
            return out
        assert op != "s_endpgm", "no barrier in the kernel"
    raise AssertionError("the kernel's end was not found")


def test_the_listing_is_the_kernel_and_has_a_barrier(listing):
    ins = front_stretch(listing)
    assert ins[-1][0] == "s_barrier" and len(ins) > 40
    assert hist_kernarg_offset(listing) % 8 == 0


def test_no_backward_branch_in_front_of_the_first_barrier(listing):
    ins = front_stretch(listing)
    at = {name: k for k, (op, name, _) in enumerate(ins) if op == "label"}
    branches = [(k, ops[0], line) for k, (op, ops, line) in enumerate(ins) if op == "s_branch" or op.startswith("s_cbranch")]
    assert branches, "the stretch holds the branch around the gated launches' second trip at the least"
    for k, target, line in branches:
        assert target in at and at[target] > k, "a loop (or a branch out of the stretch) in front of the barrier: " + line


def test_the_records_come_as_16_byte_loads_and_never_as_single_dwords(listing):
    """Registers that derive from StreamArgs::hist are followed through the (loop-free) stretch: every 16-byte load's address
    derives from it - the check sees what it is about - and no single-dword load's address does."""
    ins = front_stretch(listing)
    hist = hist_kernarg_offset(listing)
    tainted, wide, single = set(), [], []
    for op, ops, line in ins:
        if op == "label" or not ops:
            continue
        if op.startswith("s_load_dword"):
            assert ops[1] == "s[0:1]", "kernel arguments are read through s[0:1]: " + line
            dest = sorted(regs_of(ops[0]))
            off = int(ops[2], 0)
            tainted -= set(dest)
            tainted |= {r for k, r in enumerate(dest) if hist <= off + 4 * k < hist + 8}
            continue
        if op.startswith("global_load_dword"):
            aimed = bool(regs_of(ops[1]) & tainted)
            (wide if op == "global_load_dwordx4" else single).append((aimed, line))
            assert op in ("global_load_dwordx4", "global_load_dword"), line
            tainted -= regs_of(ops[0])
            continue
        if op.startswith(("s_cmp", "s_bitcmp", "s_waitcnt", "s_nop", "s_cbranch", "s_branch", "s_barrier", "ds_write", "global_store")) \
                or (op.startswith("v_cmp") and op.endswith("_e32")):
            continue                                   # no register result (scc, vcc, memory)
        n_dest = 2 if "_co_" in op or op.startswith(("v_mad_u64_u32", "v_mad_i64_i32")) else 1
        dest = set().union(*(regs_of(o) for o in ops[:n_dest]))
        derived = any(regs_of(o) & tainted for o in ops[n_dest:])
        tainted -= dest
        if derived:
            tainted |= dest
    assert len(wide) >= 1 and all(aimed for aimed, _ in wide), wide
    assert single, "the hand-off's two states and the channel are single dwords"
    assert not [line for aimed, line in single if aimed], "a single dword of a boundary record is loaded: %r" % single


def test_two_waits_for_memory_at_the_most_without_a_squelch_gate(listing):
    """Every way from the kernel's start to the barrier that a launch with vlen_gated == nullptr can take: a scalar branch on a
    64-bit compare with 0 goes the null pointer's way, every other branch both ways."""
    ins = front_stretch(listing)
    at = {name: k for k, (op, name, _) in enumerate(ins) if op == "label"}
    argument_pairs = {ops[0] for op, ops, _ in ins if op == "s_load_dwordx2" and ops[1] == "s[0:1]"}   # (none is reused in the stretch)

    def is_pointer_test(op, ops):
        return op in ("s_cmp_eq_u64", "s_cmp_lg_u64") and ops[1] == "0" and ops[0] in argument_pairs

    def most_waits(k, last_cmp):
        n = 0
        while True:
            op, ops, line = ins[k]
            if op == "s_barrier":
                return n
            if op == "s_waitcnt" and "vmcnt(" in line:
                n += 1
            if op.startswith("s_cmp"):
                last_cmp = (op, ops)
            if op == "s_branch":
                k = at[ops[0]]
                continue
            if op in ("s_cbranch_scc0", "s_cbranch_scc1") and last_cmp and is_pointer_test(*last_cmp):
                scc_when_null = 1 if last_cmp[0] == "s_cmp_eq_u64" else 0
                taken = (op == "s_cbranch_scc1") == (scc_when_null == 1)
                k = at[ops[0]] if taken else k + 1
                continue
            if op.startswith("s_cbranch"):
                return n + max(most_waits(at[ops[0]], last_cmp), most_waits(k + 1, last_cmp))
            k += 1

    assert sum(is_pointer_test(op, ops) for op, ops, _ in ins if op != "label") == 1   # vlen_gated: the one pointer the stretch asks about
    assert most_waits(0, None) <= 2
