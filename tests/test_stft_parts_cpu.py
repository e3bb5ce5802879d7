"""CPU-side checks of everything around the STFT family's kernels (no GPU): the parts of csrc/vp_stft.hip and their order, what the
build derives from the include lines, and -- from the built library's code objects (tools/kernel_resources.py) and its size functions --
the budgets of every derived kernel.  One row of KERNELS per derived kernel, one entry of FIGURES per pinned parent; a new part is one
name in PARTS and one row per kernel."""
import ast
import collections
import ctypes as C
import difflib
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "vocoderproject_amd", "csrc")

# the parts vp_stft.hip includes, in order: a part stands behind the parts whose helpers it uses (the comment above the list in vp_stft.hip)
PARTS = ["vp_stft_curve.inc", "vp_stft_stretch.inc", "vp_stft_lock.inc", "vp_stft_lockf.inc", "vp_stft_harm.inc",
         "vp_stft_stretch_lock.inc", "vp_stft_cross.inc", "vp_stft_onset.inc", "vp_stft_stretch_reset.inc", "vp_stft_formant.inc"]

LDS_CEILING = 160 * 1024 - 512
assert LDS_CEILING == 163328
CEILING_REQUEST = "hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512"
FUSED, FUSED_PLAIN = "vp_k_stft_fused<true, false>", "vp_k_stft_fused<false, false>"

# (vgpr, agpr) of the kernels the derived ones were copied from: a copy exists so that these do not move
FIGURES = {FUSED: (341, 85), "vp_k_stft_pv_curve": (346, 90), "vp_k_stft_pv_stretch": (346, 90), "vp_k_stft_pv_lock": (361, 105),
           "vp_k_stft_pv_stretch_lock": (361, 105), "vp_k_pv_stream": (337, 81), "vp_k_pv_stream_curve": (334, 78)}

# part: the file the kernel is in.  parents: the kernel it is a copy of, then that kernel's ancestors (all still built, without scratch).
# mark, marks: what differs from the parent carries this mark, at least so many times in the file.  poison: VP_POISON_LDS prologues in
# the file.  launch: the launcher's kernel, grid, block and dynamic-LDS expression.  ceiling: the part requests 160 * 1024 - 512 bytes of
# dynamic LDS for this kernel.  regs: SUM = no scratch, no vector spill, vgpr + agpr <= 512; VGPR = no scratch, vgpr <= 512 (on this
# target the metadata's vgpr_count already contains the AGPRs, so SUM asks more than the hardware does).  None: not asserted.
Row = collections.namedtuple("Row", "kernel part parents mark marks poison launch ceiling regs")
SUM, VGPR = "vgpr + agpr <= 512, no vector spill", "vgpr <= 512"
STREAM = "dim3(a.S), dim3(64 * NWV)"
KERNELS = [
    Row("vp_k_stft_pv2k", "vp_stft.hip", (), None, 0, None, None, None, SUM),
    Row("vp_k_stft_pv_curve", "vp_stft_curve.inc", (FUSED,), None, 0, 3, "vp_k_stft_pv_curve, grid, block, lds + pv_lds_bytes()", True, SUM),
    Row("vp_k_stft_pv2k_curve", "vp_stft_curve.inc", ("vp_k_stft_pv2k",), None, 0, 3, "vp_k_stft_pv2k_curve, grid, block, lds + pv2k_lds_bytes()", True, SUM),
    Row("vp_k_pv_stream_curve", "vp_stft_curve.inc", ("vp_k_pv_stream",), None, 0, 3, f"vp_k_pv_stream_curve, {STREAM}, vp_pv_lds_bytes()", True, SUM),
    Row("vp_k_stft_pv_stretch", "vp_stft_stretch.inc", (FUSED,), None, 0, 2, "vp_k_stft_pv_stretch, grid, block, lds + pv_lds_bytes()", True, SUM),
    Row("vp_k_stft_pv2k_stretch", "vp_stft_stretch.inc", ("vp_k_stft_pv2k",), None, 0, 2, "vp_k_stft_pv2k_stretch, grid, block, lds + pv2k_lds_bytes()", True, SUM),
    Row("vp_k_stft_pv_lock", "vp_stft_lock.inc", ("vp_k_stft_pv_curve", FUSED), "lock:", 10, 2, "vp_k_stft_pv_lock, grid, block, vp_stft_lock_lds_bytes(a.hop)", True, SUM),
    Row("vp_k_pv_stream_lock", "vp_stft_lock.inc", ("vp_k_pv_stream_curve", "vp_k_pv_stream"), "lock:", 10, 2, f"vp_k_pv_stream_lock, {STREAM}, vp_pv_lock_lds_bytes()", True, SUM),
    Row("vp_k_stft_pv_lockf", "vp_stft_lockf.inc", ("vp_k_stft_pv_lock",), "lockf:", 8, 2, "vp_k_stft_pv_lockf, grid, block, vp_stft_lockf_lds_bytes(a.hop)", True, SUM),
    Row("vp_k_pv_stream_lockf", "vp_stft_lockf.inc", ("vp_k_pv_stream_lock",), "lockf:", 8, 2, f"vp_k_pv_stream_lockf, {STREAM}, vp_pv_lockf_lds_bytes()", True, SUM),
    Row("vp_k_stft_harm", "vp_stft_harm.inc", ("vp_k_stft_pv_lock",), "harm:", 10, 2, "vp_k_stft_harm, grid, block, vp_stft_harm_lds_bytes(a.hop)", True, VGPR),
    Row("vp_k_hz_stream", "vp_stft_harm.inc", ("vp_k_pv_stream_lock",), "harm:", 10, 2, f"vp_k_hz_stream, {STREAM}, vp_hz_lds_bytes()", True, VGPR),
    Row("vp_k_stft_pv_stretch_lock", "vp_stft_stretch_lock.inc", ("vp_k_stft_pv_lock",), "stretch:", 10, 1, "vp_k_stft_pv_stretch_lock, grid, block, vp_stft_lock_lds_bytes(a.hop)", True, SUM),
    Row("vp_k_stft_cross", "vp_stft_cross.inc", (FUSED_PLAIN, "vp_k_stft_pv_formant"), None, 0, 2, "vp_k_stft_cross, grid, block, vp_stft_lds_bytes(a.F, a.hop, 0)", False, SUM),
    Row("vp_k_xs_stream", "vp_stft_cross.inc", ("vp_k_pv_stream",), None, 0, 2, f"vp_k_xs_stream, {STREAM}, vp_xs_lds_bytes()", False, SUM),
    Row("vp_k_stft_onset_flux", "vp_stft_onset.inc", (), None, 0, 1, None, True, SUM),
    Row("vp_k_stft_pv_stretch_lock_reset", "vp_stft_stretch_reset.inc", ("vp_k_stft_pv_stretch_lock",), "reset:", 8, 1,
        "vp_k_stft_pv_stretch_lock_reset, grid, block, vp_stft_lock_lds_bytes(a.hop)", True, SUM),
    Row("vp_k_stft_pv_formant", "vp_stft_formant.inc", ("vp_k_stft_pv_curve", FUSED), "formant:", 10, 2, "vp_k_stft_pv_formant, grid, block, lds + pv_lds_bytes()", True, SUM),
    Row("vp_k_pv_stream_formant", "vp_stft_formant.inc", ("vp_k_pv_stream_curve", "vp_k_pv_stream"), "formant:", 10, 2, f"vp_k_pv_stream_formant, {STREAM}, vp_pv_lds_bytes()", True, SUM),
]
IDS = [r.kernel for r in KERNELS]

# what else a part's text is held to: strings it contains, strings it must not contain, exact counts
SIG_CURVE = ("void vp_k_stft_pv_curve(VpStftArgs A, const double *ratioTab)", "void vp_k_pv_stream_curve(VpPvArgs A, const double *ratioTab)")
ONE_BLOCK = "const dim3 grid(1, nStreams), block(64 * NWV);"
TEXT = {
    "vp_stft.hip": dict(has=("void vp_k_stft_pv2k(VpStftArgs A)", "void vp_k_pv_stream(VpPvArgs A)")),
    "vp_stft_curve.inc": dict(has=SIG_CURVE, lacks=("stretch",)),                   # (the stretch kernels are a file of their own)
    # the harmonizer calls the split helpers of its own file; the locked ones stay one definition and two kernels' calls
    "vp_stft_lock.inc": dict(counts={"pv_lock_plan(": 3, "pv_lock_turn(": 3, "pv_lock_gather(": 3}),
    "vp_stft_lockf.inc": dict(counts={"asm volatile": 2}),                          # the parents' one empty statement each, nothing more
    "vp_stft_harm.inc": dict(lacks=("pv_lock_plan(", "pv_lock_turn(", "pv_lock_gather(", "while"),      # no wait that can spin
                             counts={"asm volatile": 2, "#pragma nounroll": 2}),    # the voice loop is a run-time loop in both kernels
    "vp_stft_stretch_lock.inc": dict(has=("void vp_k_stft_pv_stretch_lock(VpStftArgs A, const double *ratioTab, const int *posTab, int nIn)", ONE_BLOCK,
                                          "pv_lock_mask(", "pv_lock_nearest(", "pv_lock_turn(", "pv_lock_gather(", "pv_lock_carve(", "pv_stretch_frame(",
                                          "__device__ __forceinline__ bool pv_stretch_lock_plan(")),
    "vp_stft_cross.inc": dict(lacks=("PvLds", "pv_lds_carve", "hipFuncAttributeMaxDynamicSharedMemorySize")),   # no phase-vocoder arrays, below 64 KB
    "vp_stft_onset.inc": dict(has=("void vp_k_stft_onset_flux(VpStftArgs A, int nIn, int nG, int chunk, double *flux, double *mass)",
                                   "fft512_rx(", "rfft_split(", "stft_load_frame(", "A.win", "A.tws", "fft_lane_init("),
                              lacks=("asm",)),                                      # plain C++: fixed-order sums, ordinary vector stores
    "vp_stft_stretch_reset.inc": dict(has=("void vp_k_stft_pv_stretch_lock_reset(VpStftArgs A, const double *ratioTab, const int *posTab, int nIn, const unsigned char *resetTab)",
                                           ONE_BLOCK, "pv_lock_turn(", "pv_lock_gather(", "pv_lock_carve(", "pv_stretch_frame(", "pv_stretch_lock_plan("),
                                      lacks=("bool pv_stretch_lock_plan(", "void pv_lock_turn(")),      # used as they are, not copied
    "vp_capi.hip": dict(has=("vp_stft_lock_prepare_device() == hipSuccess && vp_stft_stretch_lock_prepare_device() == hipSuccess",
                             "vp_stft_onset_prepare_device() == hipSuccess && vp_stft_stretch_reset_prepare_device() == hipSuccess")),
    "vp_stft.h": dict(has=("#define VP_HARM_MAX_VOICES 4",)),
}


def text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import build
    return C.CDLL(build.build())


def lds_fn(lib, name, nargs=0):
    """size_t name(int, ...) of the library: a C++ symbol, so by its mangled name."""
    fn = getattr(lib, f"_Z{len(name)}{name}" + ("i" * nargs or "v"))
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int] * nargs
    return fn


# ---- the layout: one flat list, and a build that reads it from the include lines ------------------------------------------------------
def test_vp_stft_hip_includes_every_part_itself_in_this_order_and_ends_with_the_formant_part():
    src = text("vp_stft.hip")
    assert re.findall(r'^#include "(vp_(?:stft|pv)_[a-z_]+\.inc)"', src, re.M) == PARTS
    assert src.rstrip().endswith('#include "vp_stft_formant.inc"')
    assert re.search(r"template <bool PV, bool MAG>\s*__global__ __launch_bounds__\(64 \* NWV\) void vp_k_stft_fused\(VpStftArgs A\)", src)
    for inc in glob.glob(os.path.join(CSRC, "*.inc")):
        assert not re.search(r'#\s*include\s*"vp_stft_', open(inc).read()), inc     # no part enters through another part


def test_the_build_derives_its_dependencies_from_the_include_lines():
    from vocoderproject_amd import build
    deps = {s: [os.path.relpath(p, ROOT) for p in build.deps_of(s)] for s in build.SOURCES}
    for s, d in deps.items():
        assert d == sorted(d) and os.path.join("vocoderproject_amd", "csrc", s) in d, (s, d)
    names = {s: {os.path.basename(p) for p in d} for s, d in deps.items()}
    assert names["vp_stft.hip"] == set(PARTS) | {"vp_stft.hip", "vp_stft.h", "vp_fft.inc", "vp_fft32.inc"}
    assert {"vp_onset_host.inc", "vp_stft.h", "vp_amd.h"} <= names["vp_capi.hip"] and "include/vp_amd.h" in deps["vp_capi.hip"]
    assert names["vp_kernels.hip"] | {"vp_voc2.hip", "vp_voc2.h"} == names["vp_voc2.hip"] and "vp_pitch_ws_body.inc" in names["vp_kernels.hip"]
    assert set(build.DEPS) == set().union(*names.values())
    on_disk = {f for f in os.listdir(CSRC) if f.endswith((".inc", ".h", ".hip"))}
    assert on_disk <= set(build.DEPS), on_disk - set(build.DEPS)                    # a file nothing includes is a file the build cannot see


@pytest.mark.parametrize("source", ["vp_kernels.hip", "vp_voc2.hip", "vp_stft.hip", "vp_channels.hip", "vp_track.hip", "vp_capi.hip"])
def test_deps_of_names_every_repository_file_the_compiler_reads(source):
    from vocoderproject_amd import build
    assert source in build.SOURCES and len(build.SOURCES) == 6
    if not os.path.exists(build.hipcc()):
        pytest.skip("no hipcc")
    out = subprocess.run([build.hipcc(), "-std=c++17", f"--offload-arch={build.ARCH}", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-MM",
                          os.path.join(CSRC, source)], check=True, capture_output=True, text=True).stdout
    # (one make rule for the device pass and one for the host pass, in the bundler's wrapping: every word that is a file of this repository)
    read = {os.path.realpath(t) for t in out.replace("\\\n", " ").split() if os.path.isfile(t)}
    read = {p for p in read if p.startswith(os.path.realpath(ROOT) + os.sep)}
    assert os.path.realpath(os.path.join(CSRC, source)) in read
    assert read <= {os.path.realpath(p) for p in build.deps_of(source)}, read


# ---- the parts' text ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", KERNELS, ids=IDS)
def test_each_kernel_stands_in_its_part_as_its_row_says(row):
    inc = text(row.part)
    assert f"void {row.kernel}(" in inc
    if row.part in PARTS:
        assert "atomic" not in inc.lower()                     # the stages are gathers: no scatter, no LDS atomics
        assert inc.count("#ifdef VP_POISON_LDS") == row.poison == sum(r.part == row.part for r in KERNELS)      # every copy keeps the prologue
        assert inc.count(CEILING_REQUEST) == sum(r.part == row.part and r.ceiling for r in KERNELS)
    if row.mark:
        assert inc.count(row.mark) >= row.marks                # what differs from the parents is marked
    if row.launch:
        assert row.launch + ", st, a" in inc                   # (the stream follows the LDS expression: nothing is added to it)
    assert {r.part for r in KERNELS} == set(PARTS) | {"vp_stft.hip"}


@pytest.mark.parametrize("name", sorted(TEXT))
def test_each_file_keeps_what_its_feature_relies_on(name):
    inc = text(name)
    for s in TEXT[name].get("has", ()):
        assert s in inc, s
    for s in TEXT[name].get("lacks", ()):
        assert s.lower() not in inc.lower(), s
    for s, n in TEXT[name].get("counts", {}).items():
        assert inc.count(s) == n, (s, inc.count(s))
    if name == "vp_stft_stretch_lock.inc":                     # a plan of its own, not the locked one
        assert "pv_lock_plan(" not in inc.replace("pv_stretch_lock_plan(", "")
    if name == "vp_stft.h":
        assert "#define VP_HARM_MAX_VOICES 4" in open(os.path.join(ROOT, "include", "vp_amd.h")).read()


def _kernel_text(src, name):
    a = src.index(f"void {name}(")
    return src[src.index("\n", a) + 1:src.index("\n}\n", a) + 3]                      # (the body: the signature is asserted apart)


def assert_marked_copy(parent_file, parent_kernel, copy_file, copy_kernel, mark, max_lost):
    """Statement for statement: every line of the copy that is not in the parent's kernel carries the mark, and at most max_lost of the
    parent's lines are gone (a replaced parent line comes back marked)."""
    pl = _kernel_text(text(parent_file), parent_kernel).split("\n")
    cl = _kernel_text(text(copy_file), copy_kernel).split("\n")

    def code(line):
        return re.sub(r"\s+", " ", line.split("//")[0]).strip()
    unmarked_new, lost = [], []
    for tag, a0, a1, b0, b1 in difflib.SequenceMatcher(None, [code(x) for x in pl], [code(x) for x in cl], autojunk=False).get_opcodes():
        if tag in ("replace", "insert"):
            unmarked_new += [x for x in cl[b0:b1] if code(x) and mark not in x]
        if tag in ("replace", "delete"):
            lost += [x for x in pl[a0:a1] if code(x)]
    assert not unmarked_new, unmarked_new
    assert len(lost) <= max_lost, lost


def test_the_reset_kernel_is_a_marked_copy_of_the_locked_stretch():
    # (the three lost lines: the signature, the request's comment, the turn)
    assert_marked_copy("vp_stft_stretch_lock.inc", "vp_k_stft_pv_stretch_lock", "vp_stft_stretch_reset.inc", "vp_k_stft_pv_stretch_lock_reset", "reset:", 3)


# ---- the built kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", KERNELS, ids=IDS)
def test_each_kernel_is_built_without_scratch_within_512_registers(resources, row):
    assert row.kernel in resources, sorted(resources)
    r = resources[row.kernel]
    print(f"STFT PARTS resources {row.kernel} {r}")
    assert r["scratch"] == 0, r
    if row.regs == SUM:
        assert r["vgpr_spill"] == 0 and r["vgpr"] + r["agpr"] <= 512, r
    else:
        assert row.regs == VGPR and r["vgpr"] <= 512, r
    assert r["lds"] == 0, r                                    # no static LDS: everything is the dynamic carve
    for parent in row.parents:
        assert parent in resources and resources[parent]["scratch"] == 0, (parent, resources.get(parent))
    for update in ("vp_k_xs_update", "vp_k_hz_update"):        # the streams' state kernels
        assert update in resources and resources[update]["scratch"] == 0


@pytest.mark.parametrize("kernel", sorted(FIGURES))
def test_the_parents_keep_their_register_figures(resources, kernel):
    assert kernel in resources and resources[kernel]["scratch"] == 0, (kernel, resources.get(kernel))
    print(f"STFT PARTS resources parent {kernel} {resources[kernel]}")
    assert (resources[kernel]["vgpr"], resources[kernel]["agpr"]) == FIGURES[kernel], (kernel, resources[kernel])


def test_the_recorded_figures_are_the_built_ones(resources):
    want = {"pv_lock": 6, "pv_lockf": 4, "pv_harm": 5, "pv_stretch_lock": 4, "pv_transient": 7, "pv_formant": 4, "pv_cross": 7}     # rows per file
    rows = {}
    for name, n in want.items():
        txt = open(os.path.join(ROOT, "profiles", name + "_resources.txt")).read()
        rows[name] = dict(re.findall(r"^(vp_k_\S+(?: \S+>)?)\s+(\{.*\})$", txt, re.M))
        assert len(rows[name]) == n, (name, sorted(rows[name]))
        for k, rec in rows[name].items():
            assert k in resources and resources[k] == ast.literal_eval(rec), (name, k, resources.get(k), rec)
    assert {"vp_k_stft_pv_lock", "vp_k_pv_stream_lock"} <= set(rows["pv_lock"]) and {"vp_k_stft_harm", "vp_k_hz_stream"} <= set(rows["pv_harm"])
    assert set(FIGURES) <= set().union(*rows.values())


# ---- dynamic LDS: each feature's formula, from the library's own size functions -------------------------------------------------------
HOPS, HOPS_2K = (64, 128, 256, 512), (128, 256, 512, 1024)
PV_ARRAYS = (4 * 2 + 5 + 4 + 1) * 513 * 8                      # ana, phPrev, inc, sum of the 1024-point stage (PvLds)
LOCK_EXTRA = 4 * (2 * 10 * 8 + 2 * 520 * 4)                    # per wavefront two masks of 10 words, two maps of 520 ints
HARM_EXTRA = 3 * 513 * 8                                       # the angle arrays of voices 1 .. 3


def within(sizes, ceiling=LDS_CEILING, strictly=False):
    for k, b in sizes.items():
        assert 4 * 8192 < b <= ceiling - strictly, (k, b)


def test_curve_stretch_and_formant_lds_is_the_parents_and_pv2k_fits_the_ceiling(lib):
    base, pv2k, stream = lds_fn(lib, "vp_stft_lds_bytes", 3), lds_fn(lib, "vp_stft_pv2k_lds_bytes", 1), lds_fn(lib, "vp_pv_lds_bytes")
    # the streaming carve is four 8 KB exchange buffers, the ring (4096 floats) and the history (1024 floats) in front of the stage's arrays
    assert PV_ARRAYS == stream() - (4 * 8192 + (4096 + 1024) * 4) and PV_ARRAYS % (513 * 8) == 0
    sizes = {(1024, hop): base(1024, hop, 0) + PV_ARRAYS for hop in HOPS}
    sizes.update({(2048, hop): pv2k(hop) for hop in HOPS_2K})
    sizes["stream"] = stream()
    print(f"STFT PARTS dynamic LDS curve, stretch, formant {sizes}")
    within(sizes)
    for hop in HOPS_2K:
        # at least the slots, the carry and one (magnitude, frequency) pair, two phases and the accumulator per bin
        assert 4 * 8192 + (2048 - hop) * 4 + 1025 * 8 * 5 <= pv2k(hop), hop
    assert pv2k(128) > pv2k(256) > pv2k(512) > pv2k(1024)


def test_locked_lds_is_the_curve_parents_plus_the_stage_and_subbin_and_harmonizer_build_on_it(lib):
    base, stream = lds_fn(lib, "vp_stft_lds_bytes", 3), lds_fn(lib, "vp_pv_lds_bytes")
    lock, lstream = lds_fn(lib, "vp_stft_lock_lds_bytes", 1), lds_fn(lib, "vp_pv_lock_lds_bytes")
    lockf, fstream = lds_fn(lib, "vp_stft_lockf_lds_bytes", 1), lds_fn(lib, "vp_pv_lockf_lds_bytes")
    harm, hstream = lds_fn(lib, "vp_stft_harm_lds_bytes", 1), lds_fn(lib, "vp_hz_lds_bytes")
    assert lstream() - stream() == LOCK_EXTRA
    for hop in HOPS:
        assert lock(hop) == base(1024, hop, 0) + PV_ARRAYS + LOCK_EXTRA, hop
        assert lockf(hop) == lock(hop) and harm(hop) == lock(hop) + HARM_EXTRA, hop
    assert fstream() == lstream() == 144400
    assert hstream() == lstream() + HARM_EXTRA == 144400 + 12312 and harm(64) == 127760 + 12312
    sizes = {name: {**{hop: fn(hop) for hop in HOPS}, "stream": st()} for name, fn, st in (("lock", lock, lstream), ("lockf", lockf, fstream), ("harm", harm, hstream))}
    print(f"STFT PARTS dynamic LDS {sizes}")
    within(sizes["lock"])                                      # the locked stretch and its reset copy pass vp_stft_lock_lds_bytes(a.hop) too
    within(sizes["lockf"], strictly=True)
    within(sizes["harm"])


def test_cross_lds_stays_below_the_default_64_kb_and_the_onset_flux_is_five_rows(lib):
    base, xs, flux = lds_fn(lib, "vp_stft_lds_bytes", 3), lds_fn(lib, "vp_xs_lds_bytes"), lds_fn(lib, "vp_stft_onset_lds_bytes")
    sizes = {hop: base(1024, hop, 0) for hop in HOPS}
    sizes["stream"] = xs()
    print(f"STFT PARTS dynamic LDS cross {sizes} flux {flux()}")
    assert xs() == 4 * 8192 + (4096 + 2 * 1024) * 4 == 56 * 1024
    within(sizes, ceiling=64 * 1024, strictly=True)
    assert 4 * 8192 + 5 * 513 * 8 == flux() <= LDS_CEILING       # the same at every hop
