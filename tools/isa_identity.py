"""Compare the device ISA of two builds kernel by kernel: python tools/isa_identity.py OLD_DIR NEW_DIR [file.s ...]
The directories hold what tools/device_isa_fingerprint.sh writes (hipcc --offload-device-only -S, one .s per translation unit).  A kernel's body is its
instruction text between its label and its .Lfunc_end, with comments and .loc / .file / .cfi lines removed, its own symbol normalised and local label numbers
renumbered in order of appearance.  A kernel whose mangled name changed (template arguments appended) is matched to the kernel of the same function name
with the same body.  Prints one line per file, the renames, the new kernels, and a total; exit status 1 if a pre-existing kernel changed."""
import re
import sys
from pathlib import Path


def bodies(path):
    text = Path(path).read_text()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out = {}
    for name in kernels:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)
        assert m, name
        labels = {}
        lines = []
        for ln in m.group(1).split("\n"):
            ln = re.sub(r"\s*;.*$", "", ln).strip()
            if not ln or re.match(r"\.(loc|file|cfi_\w+|p2align)\b", ln):
                continue
            ln = ln.replace(name, "KERNEL")
            ln = re.sub(r"\.L(BB|tmp|func_begin)\d+(_\d+)?", lambda k: labels.setdefault(k.group(0), f".L{len(labels)}"), ln)
            lines.append(ln)
        out[name] = "\n".join(lines)
    return out


def base(name):   # _ZN5amuse12_GLOBAL__N_110k_vae_rowsILi0E... -> k_vae_rows
    m = re.search(r"(?:N_1|amuse)(\d+)", name)
    i = m.end(1)
    return name[i:i + int(m.group(1))] if m else name


def main():
    old_dir, new_dir = Path(sys.argv[1]), Path(sys.argv[2])
    files = sys.argv[3:] or sorted(p.name for p in old_dir.glob("*.s"))
    same = total = 0
    for f in files:
        old, new = bodies(old_dir / f), bodies(new_dir / f)
        used, lines, ok = set(), [], 0
        for name in sorted(old):
            cands = [name] if name in new else [n for n in sorted(new) if n not in old and n not in used and base(n) == base(name) and new[n] == old[name]]
            hit = next((n for n in cands if new[n] == old[name]), None)
            if hit:
                ok += 1
                used.add(hit)
                if hit != name:
                    lines.append(f"    SAME    {name}\n            -> {hit}")
            else:
                lines.append(f"    CHANGED {name}")
        fresh = [n for n in sorted(new) if n not in used]
        print(f"{f:18s} {len(old):3d} kernels before: {ok:3d} identical" + (f"; new: {len(fresh)}" if fresh else ""))
        for ln in lines:
            print(ln)
        for n in fresh:
            print(f"    new     {n}")
        same += ok
        total += len(old)
    print(f"total: {same} of {total} pre-existing kernels identical")
    sys.exit(0 if same == total else 1)


if __name__ == "__main__":
    main()
