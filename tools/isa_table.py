"""Static instruction counts of two builds' device code, kernel by kernel.
usage: python tools/isa_table.py <dirA> <dirB> [--filter SUBSTR]

dirA / dirB hold the units' assembly (<unit>.s from hipcc --offload-arch=gfx950 <Makefile's flags>
--cuda-device-only -S). Kernels are matched by their mangled names. Per kernel: static VALU (every v_*
instruction but the MFMAs), packed fp32 (v_pk_*_f32), v_exp_f32, v_rcp_f32, v_mfma, and the metadata's
.vgpr_count and .vgpr_spill_count. After the table: the kernels that gained a spill, crossed a VGPR
step that lowers the waves per SIMD (64, 96, 128, 168, 256 of the 512-register file), or changed
their count of v_exp_f32, v_rcp_f32 or v_mfma; exit status 1 if there is any."""
import glob
import os
import re
import subprocess
import sys

STEPS = (64, 96, 128, 168, 256)   # waves per SIMD 8, 5, 4, 3, 2 at or below; 1 above
LABEL = re.compile(r"^([A-Za-z_][\w$.]*):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")


def parse(path):
    """{kernel symbol: {valu, pk, exp, rcp, mfma, vgpr, spill}} of one assembly file."""
    code, meta, cur, sym = {}, {}, None, {}
    in_meta = False
    for line in open(path):
        if line.startswith("amdhsa.kernels:"):
            in_meta = True
            continue
        if in_meta:
            # one list entry per kernel, its own fields at four spaces (the arguments' sit deeper)
            if line.startswith("  - ."):
                sym = {}
            m = re.match(r"^(?:    |  - )\.(\w+):\s*(\S+)", line)
            if m:
                sym[m.group(1)] = m.group(2)
                if m.group(1) == "vgpr_spill_count":   # fields come in alphabetical order: the last one needed
                    meta[sym["name"]] = (int(sym["vgpr_count"]), int(sym["vgpr_spill_count"]))
            if not line.startswith(" "):
                in_meta = False
            continue
        m = LABEL.match(line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
            code[cur] = dict(valu=0, pk=0, exp=0, rcp=0, mfma=0)
            continue
        m = INSN.match(line)
        if m and cur:
            op, c = m.group(1), code[cur]
            if op.startswith("v_mfma") or op.startswith("v_smfmac"):
                c["mfma"] += 1
            elif op.startswith("v_"):
                c["valu"] += 1
                c["pk"] += bool(re.match(r"v_pk_\w+_f32", op))
                c["exp"] += op.startswith("v_exp_f32")
                c["rcp"] += op.startswith("v_rcp_f32")
    return {k: dict(code[k], vgpr=v[0], spill=v[1]) for k, v in meta.items() if k in code}


def demangle(names):
    # binutils' c++filt does not know DF16_ / DF16b: spell them as vendor types for it
    spelt = [n.replace("DF16b", "u6__bf16").replace("DF16_", "u8_Float16") for n in names]
    out = subprocess.run(["c++filt", "-p"], input="\n".join(spelt), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, (s.replace("yh::(anonymous namespace)::", "").replace("yh::", "") for s in out.split("\n"))))


def step(v):
    return sum(v > s for s in STEPS)


def main():
    da, db = sys.argv[1:3]
    flt = sys.argv[sys.argv.index("--filter") + 1] if "--filter" in sys.argv else ""
    bad = []
    print(f"{'unit':8} {'kernel':72} {'VALU':>13} {'v_pk_*_f32':>11} {'exp':>9} {'rcp':>9} {'mfma':>9} {'VGPR':>9} spill")
    tot = {}
    for pa in sorted(glob.glob(os.path.join(da, "*.s"))):
        unit = os.path.basename(pa)[:-2]
        pb = os.path.join(db, unit + ".s")
        if not os.path.exists(pb):
            continue
        a, b = parse(pa), parse(pb)
        names = demangle(sorted(set(a) & set(b)))
        for k in sorted(names, key=names.get):
            if flt and flt not in names[k]:
                continue
            x, y = a[k], b[k]
            pair = lambda f: f"{x[f]}->{y[f]}"
            print(f"{unit:8} {names[k][:72]:72} {pair('valu'):>13} {pair('pk'):>11} {pair('exp'):>9} {pair('rcp'):>9} "
                  f"{pair('mfma'):>9} {pair('vgpr'):>9} {pair('spill')}")
            t = tot.setdefault(unit, [0, 0, 0])
            t[0] += x["valu"]; t[1] += y["valu"]; t[2] += 1
            why = []
            if y["spill"] > x["spill"]:
                why.append("gained a spill")
            if step(y["vgpr"]) > step(x["vgpr"]):
                why.append("crossed a VGPR step")
            for f in ("exp", "rcp", "mfma"):
                if x[f] != y[f]:
                    why.append(f"v_{f} count changed")
            if why:
                bad.append(f"{unit} {names[k]}: {', '.join(why)}")
        for k in sorted(set(a) ^ set(b)):
            print(f"{unit:8} only in {'A' if k in a else 'B'}: {k}")
    print()
    for unit, (va, vb, n) in tot.items():
        print(f"{unit:8} {n:4d} kernels, static VALU {va} -> {vb} ({100.0 * (vb - va) / max(va, 1):+.1f} %)")
    print()
    print("conditions (no new spill, no VGPR step crossed, v_exp_f32 / v_rcp_f32 / v_mfma unchanged):",
          "hold for every kernel listed" if not bad else f"{len(bad)} kernels fail")
    for s in bad:
        print("  ", s)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
