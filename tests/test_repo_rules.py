"""Static checks of the repository's own ground rules (no GPU needed)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_only_test_infrastructure_touches_the_oracle():
    """oracle/ is the CPU checker: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
    import it -- the product (package, tools, generated sources) never does."""
    allowed = {ROOT / "bench.py", ROOT / "__graft_entry__.py"}
    pat = re.compile(r"^\s*(from\s+oracle\b|import\s+oracle\b)", re.M)
    offenders = []
    for p in list(ROOT.glob("*.py")) + list((ROOT / "gnn-builder_amd").rglob("*.py")) + list((ROOT / "tools").rglob("*.py")) + \
            list((ROOT / "gnnbuilder_amd").rglob("*.py")):
        if p in allowed:
            continue
        if pat.search(p.read_text()):
            offenders.append(str(p.relative_to(ROOT)))
    assert not offenders, offenders
    # and inside the two allowed files the import sits in the checker legs only
    bench = (ROOT / "bench.py").read_text()
    assert bench.count("from oracle import") == 1 and "def cpu_baseline" in bench
    assert bench.index("from oracle import") > bench.index("def cpu_baseline")
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert entry.index("from oracle import") > entry.index("def smoke")


def test_kernels_are_written_for_gfx950_only():
    """No compatibility layers: no CUDA/HIP dual paths, no hipify markers, no Triton."""
    src = "".join(p.read_text() for p in (ROOT / "gnn-builder_amd" / "csrc").glob("*.hip"))
    for marker in ("__HIP_PLATFORM_AMD__", "__CUDACC__", "cuda_runtime", "hipify", "triton"):
        assert marker not in src, marker
    mk = (ROOT / "gnn-builder_amd" / "csrc" / "Makefile").read_text()
    assert "--offload-arch=gfx950" in mk


def test_header_cites_the_reference_interfaces():
    """Every entry point of the C ABI says which reference interface it replaces (file:line)."""
    h = (ROOT / "include" / "gnnb_hip.h").read_text()
    assert len(re.findall(r"(model\.cpp\.jinja|model_tb\.cpp\.jinja|model\.h\.jinja|gnn_builder_lib\.h|code_gen\.py|models\.py):\d+", h)) >= 10


def test_every_unit_is_built_and_the_probe_build_follows_the_unit_list():
    """Round-5 review: the hand-written unity source of `make probe` had fallen five translation units behind the library
    (the diagnostic library no longer loaded).  The unit list is the ONE place that names the translation units: every
    csrc/*.hip is in it, and the probe target generates its unity source from it (no checked-in copy)."""
    csrc = ROOT / "gnn-builder_amd" / "csrc"
    mk = (csrc / "Makefile").read_text()
    units = re.search(r"^UNITS := (.*)$", mk, re.M).group(1).split()
    on_disk = sorted(p.stem for p in csrc.glob("*.hip"))
    assert sorted(units) == on_disk, (sorted(units), on_disk)
    assert not (csrc / "gnnb_unity.hip").exists()
    probe = mk[mk.index("$(OBJDIR)/gnnb_unity.hip:"):]
    assert "for u in $(UNITS)" in probe and "$(OBJDIR)/gnnb_unity.hip" in probe[probe.index("probe:"):]
    # (what the recipe writes, without running hipcc: one #include per unit, in order)
    import subprocess
    out = subprocess.run(["make", "-C", str(csrc), "-n", "probe"], capture_output=True, text=True).stdout
    assert "-DGNNB_PROBE" in out and "gnnb_unity.hip" in out


def test_kernel_sources_carry_no_build_switches_beyond_the_named_ones():
    """Measured-and-dropped alternatives are deleted, not kept behind -D switches (DESIGN 8 keeps their results): the only names
    that #if / #ifdef / #ifndef / #elif may test in csrc/ are the diagnostic and development builds' (the probe library, the ISA
    table's marks, the phase-skip build of k_gcn2_zf, the one-instantiation build) and a header's own include guard (`#ifndef X`
    followed by `#define X` at its top)."""
    allowed = {"GNNB_PROBE", "GNNB_ZF_MARK", "GNNB_ZF_ABLATE", "GNNB_DEV_FAST"}
    csrc = ROOT / "gnn-builder_amd" / "csrc"
    files = sorted(csrc.glob("*.hip")) + sorted(csrc.glob("*.h"))
    assert len(files) > 10
    offenders = []
    for p in files:
        lines = p.read_text().splitlines()
        code = [i for i, l in enumerate(lines) if l.strip() and not l.lstrip().startswith("//")]
        guard = None
        if p.suffix == ".h" and len(code) >= 2:
            m = re.match(r"\s*#\s*ifndef\s+(\w+)\s*$", lines[code[0]])
            if m and re.match(rf"\s*#\s*define\s+{m.group(1)}\s*$", lines[code[1]]):
                guard = (code[0], m.group(1))
        for i, l in enumerate(lines):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", l)
            if not m:
                continue
            expr = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
            for name in re.findall(r"[A-Za-z_]\w*", expr):
                if name != "defined" and name not in allowed and (i, name) != guard:
                    offenders.append(f"{p.name}:{i + 1}: {name}")
    assert not offenders, offenders


def test_every_header_rebuilds_the_objects_that_include_it(tmp_path):
    """A header missing from the Makefile's list left k_readout.o and the two k_stack_zf objects stale after an edit to
    gnnb_head.h.  The list is derived now: for every csrc/*.h, ``make -n -W <header>`` names at least one object to rebuild, and
    for gnnb_head.h exactly the units that include it, directly or through k_stack_zf.h.  Runs against stand-in objects in a
    scratch directory (newer than every source), so that a tree that has not been built answers the same; -n -W neither
    touches nor builds anything."""
    import subprocess
    csrc = ROOT / "gnn-builder_amd" / "csrc"
    units = re.search(r"^UNITS := (.*)$", (csrc / "Makefile").read_text(), re.M).group(1).split()
    (tmp_path / "flags.stamp").touch()
    for u in units:
        (tmp_path / f"{u}.o").touch()

    def rebuilt(header):
        out = subprocess.run(["make", "-C", str(csrc), "-n", "-W", header, "-o", str(tmp_path / "flags.stamp"), f"OBJDIR={tmp_path}",
                              f"OUT={tmp_path / 'lib.so'}"], capture_output=True, text=True, check=True).stdout
        return sorted(re.findall(r" -c -o \S*/(\w+)\.o ", out))

    assert rebuilt("no_such_header.h") == []
    headers = sorted(p.name for p in csrc.glob("*.h"))
    assert "gnnb_head.h" in headers and len(headers) > 8
    for h in headers:
        assert rebuilt(h), h
    assert rebuilt("gnnb_head.h") == ["k_readout", "k_stack_zf", "k_stack_zf_head"]
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(["flags.stamp"] + [f"{u}.o" for u in units])
