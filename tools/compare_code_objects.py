#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of libgnnb_hip.so the same machine code?  (No GPU needed.)

    tools/compare_code_objects.py OLD.so NEW.so

Both libraries are unbundled the way tests/test_register_budget.py does it (llvm-objcopy --dump-section=.hip_fatbin, split at
__CLANG_OFFLOAD_BUNDLE__, clang-offload-bundler --unbundle).  Per kernel symbol two things are compared: the raw bytes of its
function in .text (between the symbol's bounds) and its metadata note (.vgpr_count, .agpr_count, .sgpr_count,
.group_segment_fixed_size, .private_segment_fixed_size, .kernarg_segment_size, .max_flat_workgroup_size).  Nothing else of a code
object is looked at: the __hip_cuid_<hash> object changes its name with every compile, and the names of local symbols (lambda
ordinals) may shift.  A refactor that only removes dead source must leave every kernel identical: exit status 1 on any
difference -- a kernel on one side only, other bytes, other metadata --, and their names are printed."""
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "kernarg_segment_size", "max_flat_workgroup_size")


def run(*cmd, **kw):
    return subprocess.run([str(c) for c in cmd], check=True, capture_output=True, **kw)


def kernels(lib: Path, tmp: Path) -> dict:
    """{kernel name: [(sha256 of its function's bytes, byte count, metadata tuple), ...]} over every gfx950 code object in `lib`
    (a template instantiated in two translation units is a weak symbol in both code objects: one entry each), the entries of a
    name sorted -- a multiset: which translation unit holds a copy, and so the bundle order, is not the kernels' business."""
    fat = tmp / "fat.bin"
    run(LLVM / "llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib, tmp / "unused.so")
    data = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = {}
    for i, a in enumerate(starts):
        blob = tmp / f"bundle{i}.bin"
        blob.write_bytes(data[a:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = tmp / f"dev{i}.co"
        r = subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={blob}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
        if r.returncode != 0 or not co.exists() or co.stat().st_size == 0:
            continue
        meta = {}
        notes = run(LLVM / "llvm-readelf", "--notes", co, text=True).stdout
        for entry in notes.split("\n  - ")[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry)
            if not name or ".vgpr_count:" not in entry:
                continue
            vals = []
            for key in META:
                m = re.search(rf"\.{key}:\s+(\d+)", entry)
                vals.append(int(m.group(1)) if m else None)
            meta[name.group(1)] = tuple(vals)
        # .text as raw bytes, and where it is mapped: a function's bytes are [value - text address, + size) of that file
        text = tmp / f"text{i}.bin"
        run(LLVM / "llvm-objcopy", "-O", "binary", "--only-section=.text", co, text)
        tbytes = text.read_bytes()
        sections = run(LLVM / "llvm-readelf", "-S", "-W", co, text=True).stdout
        m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+[0-9a-f]+\s+([0-9a-f]+)", sections)
        taddr, tsize = int(m.group(1), 16), int(m.group(2), 16)
        assert tsize == len(tbytes), (co, tsize, len(tbytes))
        syms = run(LLVM / "llvm-readelf", "-s", "-W", co, text=True).stdout
        seen = set()  # (.dynsym and .symtab both list a kernel)
        for line in syms.splitlines():
            f = line.split()
            if len(f) == 8 and f[3] == "FUNC" and f[7] in meta and f[7] not in seen:
                seen.add(f[7])
                value, size = int(f[1], 16), int(f[2], 0)
                body = tbytes[value - taddr:value - taddr + size]
                assert len(body) == size and size > 0, (f[7], value, size)
                out.setdefault(f[7], []).append((hashlib.sha256(body).hexdigest(), size, meta[f[7]]))
        missing = set(meta) - set(out)
        assert not missing, f"{co}: kernels without a function symbol: {sorted(missing)[:3]}"
    return {k: sorted(v, key=repr) for k, v in out.items()}


def main() -> int:
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        old, new = kernels(Path(sys.argv[1]), Path(ta)), kernels(Path(sys.argv[2]), Path(tb))
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    both = set(old) & set(new)
    code = sorted(k for k in both if [e[:2] for e in old[k]] != [e[:2] for e in new[k]])
    meta = sorted(k for k in both if [e[2] for e in old[k]] != [e[2] for e in new[k]])
    for what, names in (("only in OLD", only_old), ("only in NEW", only_new), ("other bytes", code), ("other metadata", meta)):
        for k in names:
            detail = ""
            if what == "other bytes":
                detail = f"  ({[e[1] for e in old[k]]} -> {[e[1] for e in new[k]]} bytes)"
            elif what == "other metadata":
                detail = f"  {META}: {[e[2] for e in old[k]]} -> {[e[2] for e in new[k]]}"
            print(f"{what}: {k}{detail}")
    differing = len(set(only_old) | set(only_new) | set(code) | set(meta))
    copies = lambda d: sum(len(v) for v in d.values())
    print(f"kernel names: {len(old)} in OLD, {len(new)} in NEW ({copies(old)} / {copies(new)} functions over all code objects); differing: {differing}")
    return 1 if differing or not old else 0


if __name__ == "__main__":
    sys.exit(main())
