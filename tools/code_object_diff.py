"""Per-symbol difference of two AMDGPU code objects (CPU only; needs ROCm's llvm-objdump and
llvm-readelf, no GPU):

    python tools/code_object_diff.py A.elf B.elf [-v]

A and B are plain device ELFs, e.g. one kernel source built at two commits with the project's
flags (distributedtensorflowexample_amd/_build.py: ``common`` + HIP_FILE_FLAGS) plus
``--offload-device-only --no-gpu-bundle-output``.  For every function symbol of the text section
the disassembly is compared with the addresses stripped (mnemonics, operands and encodings
stay; the zero padding between symbols, which depends on their order, is skipped), and for
every kernel its entry of the code-object metadata note (kernarg layout,
SGPR / VGPR counts, LDS, scratch).  Prints the symbols that exist on one side only and the ones
that differ (-v: a unified diff of each), then one summary line; exit status 1 on any difference.
That is how a source move is shown to leave the device code alone."""
import difflib
import os
import re
import shutil
import subprocess
import sys


def tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/lib/llvm/bin", "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    found = shutil.which(name)
    if not found:
        sys.exit("%s not found (set ROCM_PATH)" % name)
    return found


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


LABEL = re.compile(r"^[0-9a-f]+ <(.+)>:$")
ADDR = re.compile(r"//\s*[0-9A-Fa-f]+:")  # the instruction's own address in the trailing comment


def disassembly(path):
    """{symbol: [instruction lines without addresses]}"""
    out, cur = {}, None
    for line in run(tool("llvm-objdump"), "-d", path).splitlines():
        m = LABEL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":  # ("...": zero padding)
            cur.append(ADDR.sub("//", line).strip())
    return out


def metadata(path):
    """{kernel symbol: [lines of its amdhsa.kernels entry]}"""
    entries, inside = [], False
    for line in run(tool("llvm-readelf"), "--notes", path).splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and line.startswith("  - "):  # a new entry of the kernel list
            entries.append([line])
        elif inside and line.startswith("  "):
            entries[-1].append(line)
        else:
            inside = False
    named = {}
    for entry in entries:
        sym = next(l.split(":", 1)[1].strip() for l in entry if l.strip(" -").startswith(".symbol:"))
        named[sym[:-3] if sym.endswith(".kd") else sym] = entry
    return named


def compare(what, a, b, verbose):
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(s for s in set(a) & set(b) if a[s] != b[s])
    for s in only_a:
        print("%s: only in A: %s" % (what, s))
    for s in only_b:
        print("%s: only in B: %s" % (what, s))
    for s in differ:
        print("%s: differs: %s" % (what, s))
        if verbose:
            print("\n".join(difflib.unified_diff(a[s], b[s], "A", "B", lineterm="", n=2)))
    print("%s: %d symbols in A, %d in B, %d compared, %d only in A, %d only in B, %d differ"
          % (what, len(a), len(b), len(set(a) & set(b)), len(only_a), len(only_b), len(differ)))
    return len(only_a) + len(only_b) + len(differ)


def main():
    args = [x for x in sys.argv[1:] if x != "-v"]
    if len(args) != 2:
        sys.exit(__doc__)
    verbose = "-v" in sys.argv[1:]
    bad = compare("disassembly", disassembly(args[0]), disassembly(args[1]), verbose)
    bad += compare("metadata", metadata(args[0]), metadata(args[1]), verbose)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
