#!/bin/bash
# Opcode histograms of k_dsmp's step bodies (the DBL step, the mixed step and its ADD-only
# instance) and the per-step bookkeeping outside them, separately for the DBL path and the
# mixed path, for a build.  usage: tools/isa_pool.sh [extra hipcc -D flags...]
set -e
D=$(mktemp -d)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -o $D/k.s \
  "$(dirname $0)/../firedancer_amd/csrc/fd_ed25519_kernels.hip" -I"$(dirname $0)/../firedancer_amd/csrc" "$@" 2>/dev/null
python3 - $D/k.s <<'PY'
import re, sys, collections
s = open(sys.argv[1]).read().split("\n")
i = next(n for n, l in enumerate(s) if re.match(r"^_Z\d+k_dsmp\w*:", l))
j = next(n for n in range(i, len(s)) if "s_endpgm" in s[n])
body = s[i:j + 1]
meta = "\n".join(s[j:j + 200])
print("k_dsmp vgpr %s occ %s lds %s scratch %s" % (re.search(r"; NumVgprs: (\d+)", meta).group(1),
      re.search(r"; Occupancy: (\d+)", meta).group(1), re.search(r"; LDSByteSize: (\d+)", meta).group(1),
      re.search(r"; ScratchSize: (\d+)", meta).group(1)))
# basic blocks in layout order (labelled, or the assembler's "; %bb.N" comments), with their successors
order, blocks, succ, cur = ["entry"], {"entry": []}, collections.defaultdict(set), "entry"
for l in body:
    m = re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; %(bb\.\d+):", l)
    if m:
        last = blocks[cur][-1] if blocks[cur] else ""
        if not (last.startswith("s_branch") or last.startswith("s_endpgm")):
            succ[cur].add(m.group(1))
        cur = m.group(1); order.append(cur); blocks[cur] = []; continue
    if l.startswith("\t") and not l.strip().startswith(";") and not l.strip().startswith("."):
        blocks[cur].append(l.strip())
        t = l.split()
        if t[0].startswith("s_cbranch") or t[0] == "s_branch":
            succ[cur].add(t[1])
ops = {k: collections.Counter(x.split()[0] for x in v) for k, v in blocks.items()}
nvalu = lambda c: sum(v for k, v in c.items() if k.startswith("v_"))
# issue cost per wave64 VALU instruction from the sustained rates of tools/ubench_valu.hip
# (profiles/r01_ubench_valu.txt): 55.3-56.8 lane-ops/clk/CU for the 64-bit and multiply class,
# 84.6 for v_add_u32; other 32-bit ALU ops are taken at v_add_u32's rate (not measured)
SLOW = ("v_mad_i64_i32", "v_mad_u64_u32", "v_mul_lo_u32", "v_lshl_add_u64", "v_ashrrev_i64", "v_mul_u32_u24",
        "v_mad_i32_i24", "v_lshlrev_b64", "v_lshrrev_b64", "v_add_co_u32", "v_addc_co_u32", "v_mul_hi_u32",
        "v_mul_i32_i24", "v_mad_u32_u24", "v_fma_f64")
def cycles(c):
    slow = sum(v for kk, v in c.items() if kk.startswith("v_") and kk.split("_e32")[0].split("_e64")[0] in SLOW)
    fast = nvalu(c) - slow
    return slow, fast, slow * 4 * 64 / 55.5 + fast * 4 * 64 / 84.6
# the bodies by their MAC count: 520 = DBL; 800 = mixed, and its ADD-only instance is the one
# whose per-lane selects are folded away (a handful of v_cndmask, not ~90)
name = {}
for k in order:
    mad = ops[k]["v_mad_i64_i32"]
    if mad == 520:
        name[k] = "DBL"
    elif mad == 800:
        name[k] = "ADD-only" if sum(v for o, v in ops[k].items() if o.startswith("v_cndmask")) < 40 else "mixed"
for k in order:
    if k not in name:
        continue
    c = ops[k]
    print("%s block %s: %d VALU, %d v_mad_i64_i32" % (name[k], k, nvalu(c), c["v_mad_i64_i32"]))
    print("  " + ", ".join("%s %d" % kv for kv in c.most_common(18)))
    sl, fa, cy = cycles(c)
    print("  issue cost: %d multiply/64-bit-class VALU x 4.61 + %d 32-bit VALU x 3.03 = %.0f SIMD cycles "
          "(%.2f per VALU; 4.00 if every VALU took 4)" % (sl, fa, cy, cy / max(1, sl + fa)))
# bookkeeping per path: the blocks on a cycle of the step loop through one body and none of the
# others.  "every step": the cycle cannot avoid the block; "some steps": it can (refill, the
# drain's selection against the main phase's, blocks skipped when no lane takes them, park).
def reach(src, dead, fwd=True):
    g = succ
    if not fwd:
        g = collections.defaultdict(set)
        for a, bs in succ.items():
            for b in bs:
                g[b].add(a)
    seen, todo = set(), [src]
    while todo:
        a = todo.pop()
        for b in g[a]:
            if b not in seen and b not in dead:
                seen.add(b); todo.append(b)
    return seen
for k in order:
    if k not in name:
        continue
    dead = set(x for x in name if x != k)
    cyc = (reach(k, dead) & reach(k, dead, False)) - {k}
    always = [b for b in cyc if k not in reach(k, dead | {b})]
    some = [b for b in cyc if b not in always]
    tot = lambda bs, p: sum(v for b in bs for o, v in ops[b].items() if o.startswith(p))
    print("%s path bookkeeping outside the body: every step %d VALU, %d SALU, %d LDS; some steps %d VALU more"
          % (name[k], tot(always, "v_"), tot(always, "s_"), tot(always, "ds_"), tot(some, "v_")))
over = collections.Counter()
for k in order:
    if k not in name:
        over.update(ops[k])
print("all blocks outside the bodies: %d VALU, %d SALU, %d LDS" % (
    nvalu(over), sum(v for k, v in over.items() if k.startswith("s_")), sum(v for k, v in over.items() if k.startswith("ds_"))))
PY
rm -rf $D
