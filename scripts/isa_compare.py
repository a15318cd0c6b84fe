#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 listings of two builds of csrc/ (build.sh keeps them as build/<file>-hip-amdgcn-amd-amdhsa-gfx950.s).
Per kernel: IDENTICAL (same instructions after renumbering labels and dropping comments, same resources), or before -> after of the
instruction count, registers, LDS, scratch, the compiler's occupancy, the counts that stand for the arithmetic (MFMA, v_exp, v_rcp,
transposing LDS reads, barriers, floating-point VALU lanes) and the register-limited waves per SIMD.  A VALU lane is one
v_{add,sub,mul,fma,max}_f32, two for a v_pk_ form; v_fmac_f32 is the two-address encoding of v_fma_f32 (the register allocator picks
it when the addend's register is free to be overwritten) and counts as one fma -- fp_strict leaves it out.  Exit status 1 if a condition fails:
scratch, a changed LDS size or arithmetic count, fewer register-limited waves, or a changed kernel outside the files named with --changed.
usage: python scripts/isa_compare.py OLD_BUILD_DIR NEW_BUILD_DIR [--changed attention,qproj_xattn]"""
import collections
import glob
import os
import re
import sys

COUNTED = ("v_mfma", "v_exp_f32", "v_rcp_f32", "ds_read_b64_tr_b16", "s_barrier")
INFO = dict(vgpr="TotalNumVgprs", sgpr="TotalNumSgprs", lds="LDSByteSize", scratch="ScratchSize", occ="Occupancy")


def kernels(path):
    """name -> (instructions with labels renumbered, resource dict); only symbols followed by a 'Kernel info' block are kernels"""
    out, name, body, info = {}, None, None, None
    for line in open(path):
        m = re.match(r"^(_Z[\w.$]*):", line)
        if m:
            name, body, info = m.group(1), [], None
            continue
        if name is None:
            continue
        if info is None:
            if line.startswith("; Kernel info:"):
                info = {}
            elif line.startswith(".Lfunc_end"):
                body.append(None)        # end of the instructions
            elif body and body[-1] is None:
                pass
            else:
                s = line.split(";")[0].strip()
                if s and (not s.startswith(".") or s.startswith(".LBB")):
                    body.append(s)
            continue
        for key, tag in INFO.items():
            m = re.match(r"; %s: (\d+)" % tag, line)
            if m:
                info[key] = int(m.group(1))
        if "occ" in info:
            ids = {}
            ins = [re.sub(r"\.LBB\d+_\d+", lambda m: ids.setdefault(m.group(0), "L%d" % len(ids)), s) for s in body[:-1]]
            out[name] = (ins, info)
            name = None
    return out


def counts(ins):
    c = collections.Counter()
    for s in ins:
        op = s.split()[0]
        for k in COUNTED:
            if op.startswith(k):
                c[k] += 1
        m = re.match(r"v_(pk_)?(add|sub|mul|fma|fmac|max)_f32", op)
        if m:
            c["fp_lanes"] += 2 if m.group(1) else 1
            c["fp_strict"] += 0 if m.group(2) == "fmac" else 2 if m.group(1) else 1
    c["instr"] = sum(1 for s in ins if not s.endswith(":"))
    return c


def waves(vgpr):
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def main():
    old_dir, new_dir = sys.argv[1:3]
    changed = sys.argv[sys.argv.index("--changed") + 1].split(",") if "--changed" in sys.argv else []
    bad, same, total = [], 0, 0
    for old_s in sorted(glob.glob(os.path.join(old_dir, "*-gfx950.s"))):
        src = os.path.basename(old_s).split("-hip-")[0]
        old, new = kernels(old_s), kernels(os.path.join(new_dir, os.path.basename(old_s)))
        print("== %s: %d kernels" % (src, len(old)))
        if set(old) != set(new):
            bad.append("%s: kernel symbols differ: %s" % (src, sorted(set(old) ^ set(new))))
        for k in sorted(set(old) & set(new)):
            (a, ia), (b, ib) = old[k], new[k]
            total += 1
            if a == b and ia == ib:
                same += 1
                print("IDENTICAL  %s  %d instr, %d VGPRs, %d waves" % (k, counts(a)["instr"], ia["vgpr"], waves(ia["vgpr"])))
                continue
            ca, cb = counts(a), counts(b)
            wa, wb = waves(ia["vgpr"]), waves(ib["vgpr"])
            print("DIFFERENT  %s" % k)
            print("           instr %d -> %d; VGPRs %d -> %d; SGPRs %d -> %d; LDS %d -> %d; scratch %d -> %d; Occupancy %d -> %d; reg-limited waves %d -> %d"
                  % (ca["instr"], cb["instr"], ia["vgpr"], ib["vgpr"], ia["sgpr"], ib["sgpr"], ia["lds"], ib["lds"], ia["scratch"], ib["scratch"],
                     ia["occ"], ib["occ"], wa, wb))
            print("           " + "; ".join("%s %d -> %d" % (c, ca[c], cb[c]) for c in COUNTED + ("fp_lanes", "fp_strict")))
            if src not in changed:
                bad.append("%s: changed outside %s" % (k, changed))
            if ia["scratch"] or ib["scratch"] or ia["lds"] != ib["lds"]:
                bad.append("%s: scratch / LDS" % k)
            if any(ca[c] != cb[c] for c in COUNTED + ("fp_lanes",)):
                bad.append("%s: arithmetic counts moved" % k)
            if wb < wa:
                bad.append("%s: register-limited waves per SIMD %d -> %d" % (k, wa, wb))
    print("%d of %d kernels identical" % (same, total))
    for line in bad:
        print("FAILED  " + line)
    print("conditions: %s" % ("FAILED" if bad else "all met"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
