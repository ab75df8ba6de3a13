"""Per-kernel resource metadata (VGPRs, SGPRs, scratch, spills, LDS) of every gfx950 kernel inside a built shared library.
Reads the code objects out of the .hip_fatbin section (no GPU needed).  Used by tests/test_build_resources.py and by hand:
  python3 tools/kernel_metadata.py embree-compressed_amd/lib/libembree3.so [regex]
  python3 tools/kernel_metadata.py --digest embree-compressed_amd/lib/libembree3.so [regex]
--digest prints, per kernel, a SHA-256 over its disassembled instructions (mnemonics and operands; no addresses, no encodings):
two builds whose digests agree run the same code in that kernel, wherever the kernel lies in its code object."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [o.replace("rtamd::dev::", "").replace("(rtamd::LaunchParams)", "").replace("void ", "") for o in out[: len(names)]]


def _instruction_digests(co):
    """-> {mangled symbol: sha256 over the symbol's instruction text}.  Dropped: addresses, encodings, and what depends on where the
    kernel and its constants lie in the code object - the `<symbol+offset>` note of a branch (its relative operand stays) and the
    literal of the add / addc pair that follows s_getpc_b64 (a pc-relative address of a __constant__ object)."""
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True).stdout
    out, cur, pcrel = {}, None, []
    for line in txt.split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<(.*)>:$", line)
        if m:
            cur = hashlib.sha256()
            out[m.group(1)] = cur
            pcrel = []
            continue
        ins = line.split("//")[0].split("<")[0].strip()
        if cur is None or not ins or ins == "...":  # (... = zero padding behind the last instruction)
            continue
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", ins)
        if m:  # the add / addc on exactly this register pair, directly behind it
            pcrel = ["s_add_u32 s%s, s%s," % (m.group(1), m.group(1)), "s_addc_u32 s%s, s%s," % (m.group(2), m.group(2))]
        elif pcrel and ins.startswith(pcrel[0]):
            ins = pcrel.pop(0) + " <pcrel>"
        else:
            pcrel = []
        cur.update((" ".join(ins.split()) + "\n").encode())
    return {k: h.hexdigest() for k, h in out.items()}


def kernel_metadata(lib_path, disassemble=(), digest=False):
    """-> {demangled kernel name: {vgpr, sgpr, scratch, sgpr_spills, vgpr_spills, lds, max_wg}}; for the kernels whose demangled
    names are listed in `disassemble` also "scratch_ops": number of scratch_load / scratch_store instructions in the ISA; with
    `digest` also "digest" (see _instruction_digests)."""
    res = {}
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib_path, os.path.join(td, "copy.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, s in enumerate(starts):  # one bundle per .hip translation unit
            part = os.path.join(td, "bundle%d" % i)
            open(part, "wb").write(blob[s : starts[i + 1] if i + 1 < len(starts) else len(blob)])
            co = os.path.join(td, "co%d.elf" % i)
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + part, "--output=" + co])
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
            cur = {}
            entries = []
            for line in notes.split("\n"):
                m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)\s*$", line)
                if not m:
                    continue
                k, val = m.group(1), m.group(2)
                if k in ("group_segment_fixed_size", "private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count",
                         "max_flat_workgroup_size", "agpr_count"):
                    cur[k] = int(val)
                elif k == "name" and val.startswith("_Z"):
                    cur["name"] = val
                elif k == "wavefront_size":  # last key of a kernel's (alphabetically sorted) metadata map
                    entries.append(cur)
                    cur = {}
            names = _demangle([e.get("name", "?") for e in entries])
            digests = _instruction_digests(co) if digest else {}
            for e, n in zip(entries, names):
                ops = None
                if n in disassemble:
                    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=" + e["name"], co], capture_output=True, text=True).stdout
                    ops = len(re.findall(r"\bscratch_(?:load|store)", dis))
                res[n] = dict(scratch_ops=ops, digest=digests.get(e.get("name")), vgpr=e.get("vgpr_count", 0), agpr=e.get("agpr_count", 0), sgpr=e.get("sgpr_count", 0), scratch=e.get("private_segment_fixed_size", 0),
                              sgpr_spills=e.get("sgpr_spill_count", 0), vgpr_spills=e.get("vgpr_spill_count", 0), lds=e.get("group_segment_fixed_size", 0),
                              max_wg=e.get("max_flat_workgroup_size", 0))
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--digest"]
    digest = len(args) < len(sys.argv) - 1
    pat = args[1] if len(args) > 1 else ""
    for n, r in sorted(kernel_metadata(args[0], digest=digest).items()):
        if not re.search(pat, n):
            continue
        if digest:
            print("%s  %s" % (r["digest"], n))
        else:
            print("%-90s vgpr %3d sgpr %3d scratch %4d spills s%d/v%d lds %d" % (n, r["vgpr"], r["sgpr"], r["scratch"], r["sgpr_spills"], r["vgpr_spills"], r["lds"]))
