"""compare_device_code.py <parent libmovba.so> <branch libmovba.so> [out.json]: the gfx950 code objects of two builds of the
library, kernel by kernel.  Extracts the code objects and disassembles them with the ROCm LLVM tools, and compares every
kernel symbol's instruction stream (addresses and encodings dropped; the literal of an s_add_u32 / s_addc_u32 pair behind
s_getpc_b64 is the distance to a constant table, which moves when another kernel of the same file changes size, and is
masked).  Prints the symbols that differ; the json holds every symbol compared."""
import json, os, re, shutil, subprocess, sys, tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def kernels(lib):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=tmp, stdout=subprocess.DEVNULL)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            co = os.path.join(tmp, f)
            syms = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", co], text=True)
            kds = {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.rstrip().endswith(".kd")}
            dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
            name, pc_rel = None, 0
            for ln in dis.splitlines():
                m = re.match(r"^[0-9a-f]* ?<(.+)>:$", ln.strip())
                if m:
                    name = m.group(1) if m.group(1) in kds else None
                    if name:
                        assert name not in out, name
                        out[name] = []
                    continue
                ins = ln.split("//")[0].strip()
                if not name or not ins:
                    continue
                if ins.startswith("s_getpc_b64"):
                    pc_rel = 3
                elif pc_rel and re.match(r"s_addc?_u32 ", ins):
                    ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "PCREL", ins)
                pc_rel = max(pc_rel - 1, 0)
                out[name].append(ins)
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
differ = sorted(k for k in a if k in b and a[k] != b[k])
res = {"compared": sorted(set(a) & set(b)), "identical": len(set(a) & set(b)) - len(differ), "differ": differ,
       "only_parent": sorted(set(a) - set(b)), "only_branch": sorted(set(b) - set(a)),
       "instructions": {k: [len(a[k]), len(b[k])] for k in differ}}
print(len(res["compared"]), "kernels compared,", res["identical"], "identical")
for k in differ:
    print("  differs:", k, res["instructions"][k])
for k in res["only_parent"] + res["only_branch"]:
    print("  in one build only:", k)
if len(sys.argv) > 3:
    json.dump(res, open(sys.argv[3], "w"), indent=1)
