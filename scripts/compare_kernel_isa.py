"""Compare the gfx950 instruction streams of the kernels two builds of one object file hold (e.g. ingest.o of two commits):
python scripts/compare_kernel_isa.py OLD.o NEW.o[,NEW2.o ...] [name-substring | OLDNAME=NEWNAME ...]
(several NEW objects, comma-separated: kernels that moved to a file of their own are looked up in all of them; OLDNAME=NEWNAME, both
mangled names in full: a kernel whose signature changed, e.g. by a new template parameter, is compared under its new name;
--ignore-kernarg-offsets: the offsets of the scalar loads from the kernel-argument segment, s[0:1], are left out of the comparison,
which a new trailing argument moves for the hidden arguments behind it)

Each object's device code is unbundled (clang-offload-bundler) and disassembled (llvm-objdump); per kernel present in OLD the
instructions are compared with branch-target labels and the trailing alignment padding stripped.  Exit status 1 when a kernel differs,
is missing from NEW, or exists only in NEW."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(obj, tmp):
    fat, co = os.path.join(tmp, os.path.basename(obj) + ".fat"), os.path.join(tmp, os.path.basename(obj) + ".gfx950")
    subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=" + fat, obj], check=True, stderr=subprocess.DEVNULL)
    if not os.path.exists(fat):   # (host code only, e.g. densemap_export.o: the object has no such section and holds no kernel)
        return {}
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET,
                    "--output=" + co], check=True)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"<[^>]*>", "", line.split("//")[0]).strip())
    for ins in out.values():   # (the padding up to the next kernel depends on what follows)
        while ins and ins[-1] in ("s_nop 0", "s_code_end", "..."):
            ins.pop()
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--ignore-kernarg-offsets"]
    old_obj, new_obj = args[0], args[1]
    renamed = dict(a.split("=", 1) for a in args[2:] if "=" in a)
    pats = [a for a in args[2:] if "=" not in a] + list(renamed)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "old"))
        a, b = kernels(old_obj, os.path.join(tmp, "old")), {}
        for k, obj in enumerate(new_obj.split(",")):
            os.makedirs(os.path.join(tmp, f"new{k}"))
            b.update(kernels(obj, os.path.join(tmp, f"new{k}")))
    if len(args) < len(sys.argv) - 1:
        for ks in (a, b):
            for name in ks:
                ks[name] = [re.sub(r"^(s_load_dword\w* s\S+ s\[0:1\], )0x[0-9a-f]+$", r"\1<offset>", i) for i in ks[name]]
    for old, new in renamed.items():   # (the new kernel is looked at under the old one's name)
        if new in b:
            b[old] = b.pop(new)
    bad = 0
    for name in sorted(set(b) - set(a)):
        if not pats or any(p in name for p in pats):
            bad += 1
            print("ONLY IN NEW " + name, 0, len(b[name]))
    for name in sorted(a):
        if pats and not any(p in name for p in pats):
            continue
        same = a[name] == b.get(name)
        bad += not same
        print(("identical " if same else "DIFFERENT ") + name, len(a[name]), len(b.get(name, [])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
