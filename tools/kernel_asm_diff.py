"""Per-kernel comparison of two builds' device assembly: tools/kernel_asm_diff.py DIR_BEFORE DIR_AFTER [--shrunk-args NAME:OLD:NEW]

DIR_* hold one .s file per translation unit, made with the Makefile's per-file flags plus
`--cuda-device-only --no-gpu-bundle-output -S`.  For every kernel symbol present on both sides the
instruction stream with its .amdhsa_* descriptor and the metadata note are compared after dropping comments and normalising what
depends on layout only (the __hip_cuid_* symbol, the function counter in .LBB<n>_<m> labels).  Kernels that disappeared are listed,
new ones count as differences.  --shrunk-args CompBwdArgs:224:216 declares one expected difference: kernels whose mangled name
contains NAME take an argument block that shrank from OLD to NEW bytes, which moves the hidden arguments behind it; the BEFORE side
is shifted accordingly (offsets in s_load_dword / s_add_u32, .offset / .size / .kernarg_segment_size) before the comparison.
Exit status 1 when anything else differs."""
import difflib
import os
import re
import sys


def norm(line):
    line = re.sub(r"__hip_cuid_\w+", "__hip_cuid_X", line)
    line = re.sub(r"\s*;.*$", "", line)
    return re.sub(r"\.L([A-Za-z_]+)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)


def split(path):
    """-> ({symbol: code lines up to .end_amdhsa_kernel}, {symbol: metadata lines})"""
    code, meta, cur, entry, in_meta = {}, {}, None, [], False

    def flush():
        names = [m.group(1) for m in (re.match(r"    \.name:\s+(\S+)", e) for e in entry) if m]
        if names:
            meta[names[0]] = entry[:]

    for raw in open(path).read().split("\n"):
        if raw.strip() == "amdhsa.kernels:":
            in_meta, cur = True, None
        elif in_meta:
            if raw.startswith("  - "):
                flush()
                entry = [norm(raw)]
            elif raw.startswith("    "):
                entry.append(norm(raw))
            else:
                flush()
                entry, in_meta = [], False
        else:
            m = re.match(r"\s*\.type\s+(\S+),@function", raw)
            if m:
                cur = m.group(1)
                code[cur] = []
            if cur is not None:
                if norm(raw).strip():
                    code[cur].append(norm(raw))
                if raw.strip() == ".end_amdhsa_kernel":
                    cur = None
    return code, meta


def shift(lines, old, new):
    d, out = old - new, []
    for l in lines:
        m = re.match(r"(\s*- \.offset:\s+|\s*\.kernarg_segment_size:\s+|\s*\.amdhsa_kernarg_size\s+)(\d+)$", l)
        if m and (int(m.group(2)) >= old or "offset" not in m.group(1)):
            l = m.group(1) + str(int(m.group(2)) - d)
        elif re.match(r"\s*\.size:\s+%d$" % old, l):
            l = l.replace(str(old), str(new))
        elif re.match(r"\s*(s_load_dword|s_add_u32)", l):
            # the hidden arguments a kernel reads this way (block counts, group sizes) sit within 64 bytes behind the explicit ones
            l = re.sub(r"0x[0-9a-f]+$", lambda m: hex(int(m.group(0), 16) - d) if old <= int(m.group(0), 16) < old + 64 else m.group(0), l)
        out.append(l)
    return out


def main():
    before, after = sys.argv[1], sys.argv[2]
    shrunk = sys.argv[4].split(":") if len(sys.argv) > 4 and sys.argv[3] == "--shrunk-args" else None
    bad, gone_all, n_before, n_after = 0, [], 0, 0
    for f in sorted(x for x in os.listdir(before) if x.endswith(".s")):
        (ca, ma), (cb, mb) = split(os.path.join(before, f)), split(os.path.join(after, f))
        n_before, n_after = n_before + len(ma), n_after + len(mb)
        gone, new = sorted(set(ca) - set(cb)), sorted(set(cb) - set(ca))
        gone_all += gone
        bad += len(new)
        for what, a, b in (("code", ca, cb), ("metadata", ma, mb)):
            for k in sorted(set(a) & set(b)):
                x = shift(a[k], int(shrunk[1]), int(shrunk[2])) if shrunk and shrunk[0] in k and a[k] != b[k] else a[k]
                if x is not a[k]:
                    print(f"  {f} {k}: {what} compared after the {shrunk[1]} -> {shrunk[2]} byte argument shift ({sum(p != q for p, q in zip(x, a[k]))} lines)")
                if x != b[k]:
                    bad += 1
                    d = [l for l in difflib.unified_diff(x, b[k], lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
                    print(f"  DIFFERENT {what}: {f} {k} ({len(d)} lines)")
                    for l in d[:16]:
                        print("     ", l)
        print(f"{f}: {len(ma)} -> {len(mb)} kernels, gone {gone}, new {new}")
    print(f"kernels {n_before} -> {n_after}; gone {len(gone_all)}; differing or new: {bad}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
