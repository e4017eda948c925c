#!/usr/bin/env python3
"""Do two builds of liblkhip.so hold the same device code?

    python tools/compare_device_code.py OLD.so NEW.so

Dumps the .hip_fatbin section of both libraries, unbundles every gfx950 code object (one per .hip file), disassembles each
with llvm-objdump and compares function by function: instruction text only (addresses, encodings, branch-target comments and
the padding behind a function dropped, so a function that merely moved, or became its file's last, is not reported).  Prints
the kernels / device functions that differ, or "identical".  Needs no GPU.  LLVM_BIN (default /opt/rocm/llvm/bin) names the directory of llvm-objcopy and llvm-objdump."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp, arch):
    fb = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, lib])
    data = open(fb, "rb").read()
    out, pos = [], 0
    while True:
        p = data.find(MAGIC, pos)
        if p < 0:
            return out
        n, = struct.unpack_from("<Q", data, p + 24)
        q = p + 32
        for _ in range(n):
            off, size, ts = struct.unpack_from("<QQQ", data, q)
            q += 24
            triple = data[q:q + ts].decode()
            q += ts
            if arch in triple and size:
                out.append(data[p + off:p + off + size])
        pos = p + len(MAGIC)


def functions(elf_bytes, tmp):
    f = os.path.join(tmp, "co.elf")
    open(f, "wb").write(elf_bytes)
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f], stdout=subprocess.PIPE, universal_newlines=True,
                          check=True).stdout
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*", "", line).strip())
    for body in funcs.values():     # the padding behind a function's last instruction (s_nop up to the alignment, and the
        while body and body[-1] in ("s_nop 0", "..."):  # prefetch guard behind the code object's last function) is not its code
            body.pop()
    return funcs


def main(old, new, arch="gfx950"):
    with tempfile.TemporaryDirectory() as tmp:
        a = [functions(c, tmp) for c in code_objects(old, tmp, arch)]
        b = [functions(c, tmp) for c in code_objects(new, tmp, arch)]
    fa = {k: v for co in a for k, v in co.items()}
    fb = {k: v for co in b for k, v in co.items()}
    changed = sorted(k for k in fa.keys() & fb.keys() if fa[k] != fb[k])
    print("%d code objects, %d functions in %s; %d, %d in %s" % (len(a), len(fa), old, len(b), len(fb), new))
    for title, names in (("only in old", sorted(fa.keys() - fb.keys())), ("only in new", sorted(fb.keys() - fa.keys())),
                         ("instructions differ", changed)):
        for k in names:
            print("%s: %s" % (title, k))
    same = not changed and fa.keys() == fb.keys()
    print("identical" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
