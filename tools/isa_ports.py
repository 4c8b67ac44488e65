"""Instructions of one kernel by issue port, static and along the executed blocks (for profiles/: `make asm` writes the .s file).

python tools/isa_ports.py FILE.s KERNEL-SUBSTRING [--blocks] [--layers LO:HI:P,...] [--dead LABEL[-LABEL],...]

Static: every instruction between the kernel's label and its end.  Executed: every basic block weighted by how often a wave runs
it.  A block with eight or more v_pk_fma_f32 is a term of a dense layer; --layers says how often a term runs by where its weight
row lies: a term whose first s_load offset (bytes from the stage's parameters) is in [LO, HI) weighs P (the share of live units
per 64-row group, tools/unit_sparsity.py, or 0 / 1 for a first-layer term the route does not / does run).  A block of sixteen or
more v_mov_b32 and no other VALU is the accumulators' zero fill for a dead first term, and a block of one scalar bit test and its
branch is a term's test reached from a dead term (a live term carries the next test at its end): both weigh 1 - P of the next
term in code order.  --dead lists the blocks (by number, as in .LBB72_31 -> 31; ranges by code order, both ends included; 0 is
the entry block) that the route in question does not run: weight 0.  Everything else weighs 1.  --blocks prints the table of
blocks to choose them from.
Ports: VALU (v_*), SALU (s_* arithmetic, compares, moves, bit tests), branch (s_branch, s_cbranch_*), SMEM (s_load_*), s_nop,
s_waitcnt, LDS (ds_*), VMEM (global_*, flat_*, buffer_*)."""
import re
import sys


def port(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_load_", "s_buffer_load_")):
        return "SMEM"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_setpc", "s_sleep")):
        return "branch"
    if op.startswith("s_"):
        return "SALU"
    return "other"


PORTS = ["VALU", "SALU", "branch", "SMEM", "s_nop", "s_waitcnt", "LDS", "VMEM"]


def blocks_of(path, want):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and want in l)
    out, cur = [], {"label": 0, "ops": []}
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"^\.LBB\d+_(\d+):", l)
        if m:
            out.append(cur)
            cur = {"label": int(m.group(1)), "ops": []}
            continue
        m = re.match(r"^; %bb\.(\d+):", l)
        if m and int(m.group(1)) != 0:
            out.append(cur)
            cur = {"label": int(m.group(1)), "ops": []}
            continue
        m = re.match(r"^\ts_load_dwordx(?:8|16) \S+ \S+ (0x[0-9a-f]+|\d+)", l)
        if m and "off" not in cur:
            cur["off"] = int(m.group(1), 0)
        m = re.match(r"^\t([a-z_0-9]+)", l)
        if m and (m.group(1).startswith(("v_", "s_", "ds_", "global_", "flat_", "buffer_", "scratch_"))):
            cur["ops"].append(m.group(1))
    out.append(cur)
    return out


def main():
    args = sys.argv[1:]
    path, want = args[0], args[1]
    show = "--blocks" in args
    layers = [tuple(float(x) if i == 2 else int(x, 0) for i, x in enumerate(t.split(":")))
              for t in args[args.index("--layers") + 1].split(",")] if "--layers" in args else []
    dead_spec = args[args.index("--dead") + 1].split(",") if "--dead" in args else []
    bl = blocks_of(path, want)
    order = {b["label"]: i for i, b in enumerate(bl)}
    dead = set()
    for d in dead_spec:
        lo, _, hi = d.partition("-")
        dead.update(range(order[int(lo)], order[int(hi or lo)] + 1))
    for i, b in enumerate(bl):
        b["w"], b["kind"], b["p"] = 1.0, "", None
        if b["ops"].count("v_pk_fma_f32") >= 8 and "off" in b:
            for lo, hi, pr in layers:
                if lo <= b["off"] < hi:
                    b["w"], b["kind"], b["p"] = pr, f"term @{b['off']:#x}", pr
    nxt = None   # the share of the next term in code order
    for i in range(len(bl) - 1, -1, -1):
        b = bl[i]
        if b["p"] is not None:
            nxt = b["p"]
            continue
        valu = [o for o in b["ops"] if o.startswith("v_")]
        fill = len(valu) >= 16 and all(o == "v_mov_b32" for o in valu)
        test = len(b["ops"]) == 2 and b["ops"][0].startswith("s_bitcmp") and b["ops"][1].startswith("s_cbranch")
        if nxt is not None and (fill or test):
            b["w"], b["kind"] = 1.0 - nxt, "zero fill" if fill else "test"
    for i in dead:
        bl[i]["w"], bl[i]["kind"] = 0.0, "dead"
    static = {p: 0 for p in PORTS + ["other"]}
    execd = {p: 0.0 for p in PORTS + ["other"]}
    for i, b in enumerate(bl):
        c = {p: 0 for p in PORTS + ["other"]}
        for o in b["ops"]:
            c[port(o)] += 1
        for p in c:
            static[p] += c[p]
            execd[p] += b["w"] * c[p]
        if show:
            print(f"{b['label']:5d} w={b['w']:.3f} {b['kind']:14s} " + " ".join(f"{p}={c[p]}" for p in PORTS if c[p])
                  + f"  pk_fma={b['ops'].count('v_pk_fma_f32')}")
    print("static  : " + "  ".join(f"{p} {static[p]}" for p in PORTS) + f"  | v_pk_fma_f32 {sum(b['ops'].count('v_pk_fma_f32') for b in bl)}"
          f"  v_cmp_ngt_f32 {sum(b['ops'].count('v_cmp_ngt_f32') for b in bl)}")
    print("executed: " + "  ".join(f"{p} {execd[p]:.0f}" for p in PORTS)
          + f"  | v_pk_fma_f32 {sum(b['w'] * b['ops'].count('v_pk_fma_f32') for b in bl):.0f}")


if __name__ == "__main__":
    main()
