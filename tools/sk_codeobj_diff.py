"""Compare the gfx950 code objects of two builds of sinkhorn.hip kernel by kernel, by symbol name: instruction bytes and the 64-byte kernel
descriptor (without its code-entry offset, which is a position).  A dword that differs is accepted only if it is the pc-relative literal of
g_sk_status (literal + address of the instruction = address of the variable in either object): the linker resolves it to a distance that
changes when other kernels leave .text.
    hipcc <the Makefile's flags> --cuda-device-only -c sinkhorn.hip -o a.co      (in each tree)
    python tools/sk_codeobj_diff.py a.co b.co out.json"""
import json, struct, subprocess, sys


def elf_syms(path):
    d = open(path, "rb").read()
    if d[:4] != b"\x7fELF":      # a clang offload bundle: the one gfx950 code object inside
        assert d.startswith(b"__CLANG_OFFLOAD_BUNDLE__") and d.count(b"\x7fELF\x02\x01\x01") == 1, path
        d = d[d.index(b"\x7fELF"):]
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
    secs = []
    for i in range(shnum):
        name, typ, flags, addr, off, size, link, info, align, entsize = struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize)
        secs.append(dict(name=name, type=typ, addr=addr, off=off, size=size, link=link, entsize=entsize))
    symtab = next(s for s in secs if s["type"] == 2)      # SHT_SYMTAB
    strtab = secs[symtab["link"]]
    out = {}
    for i in range(symtab["size"] // 24):
        nm, info, other, shndx, value, size = struct.unpack_from("<IBBHQQ", d, symtab["off"] + i * 24)
        if shndx == 0 or shndx >= len(secs) or size == 0:
            continue
        e = d.index(b"\0", strtab["off"] + nm)
        name = d[strtab["off"] + nm:e].decode()
        s = secs[shndx]
        if s["type"] == 8:      # NOBITS
            out[name] = (info & 15, b"", value)
            continue
        o = s["off"] + value - s["addr"]
        out[name] = (info & 15, d[o:o + size], value)
    return out


def kernels(path):
    s = elf_syms(path)
    k = {}
    for name, (typ, data, value) in s.items():
        if name.endswith(".kd") and len(data) == 64:
            fn = name[:-3]
            code = s[fn][1]
            # the descriptor's KERNEL_CODE_ENTRY_BYTE_OFFSET (bytes 16..23) is the distance descriptor -> code: position, not content
            k[fn] = (code, data[:16] + data[24:], s[fn][2])
    return k, s["_ZN2dr11g_sk_statusE"][2]


def rebased(ka, kb, ga, gb):
    """code of kernel b with every differing dword that is a pc-relative literal of g_sk_status (same distance literal + site - variable in both
    objects) replaced by a's: equal to a's code iff nothing but those literals differs"""
    (ca, _, va), (cb, _, vb) = ka, kb
    if len(ca) != len(cb):
        return cb, 0
    out, n = bytearray(cb), 0
    for o in range(0, len(ca), 4):
        if ca[o:o + 4] != cb[o:o + 4]:
            la, lb = struct.unpack("<i", ca[o:o + 4])[0], struct.unpack("<i", cb[o:o + 4])[0]
            if la + va + o - ga == lb + vb + o - gb:
                out[o:o + 4] = ca[o:o + 4]; n += 1
    return bytes(out), n


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.split("\n")[:len(names)]


(a, ga), (b, gb) = kernels(sys.argv[1]), kernels(sys.argv[2])
removed = sorted(set(a) - set(b))
added = sorted(set(b) - set(a))
differ = sorted(n for n in set(a) & set(b) if a[n][:2] != b[n][:2])
reloc = {n: rebased(a[n], b[n], ga, gb) for n in differ}
reloc_only = sorted(n for n in differ if reloc[n][0] == a[n][0] and a[n][1] == b[n][1])
differ = sorted(set(differ) - set(reloc_only))
code_differ = sorted(n for n in set(a) & set(b) if a[n][0] != b[n][0])
res = dict(parent_kernels=len(a), new_kernels=len(b), added=added, differing=demangle(differ) if differ else [], identical=len(set(a) & set(b)) - len(differ) - len(reloc_only),
           identical_but_for_the_pc_relative_address_of_g_sk_status=demangle(reloc_only), literals_rebased=sorted(set(reloc[n][1] for n in reloc_only)),
           removed=demangle(removed) if removed else [])
json.dump(res, open(sys.argv[3], "w"), indent=1)
print(json.dumps({k: (v if not isinstance(v, list) else len(v)) for k, v in res.items()}))
for n in differ[:5]:
    ca, cb = a[n][0], b[n][0]
    pos = [i for i in range(min(len(ca), len(cb))) if ca[i] != cb[i]]
    print(n, len(ca), len(cb), "differing bytes", len(pos), pos[:16], "kd equal", a[n][1] == b[n][1])
