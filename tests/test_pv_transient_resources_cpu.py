"""CPU-side check of the transient-preserving stretch's two kernels, from the built library (no GPU, no compiler run): both exist, use no
scratch, spill no vector register, fit the 512 registers a lane has at one wavefront per SIMD and have no static LDS
(tools/kernel_resources.py reads the code object's metadata); their dynamic LDS is within the ceiling at every hop and each requests the
ceiling once, where the others do; both keep the VP_POISON_LDS prologue; each is a file of its own behind the existing includes; the reset
kernel is a copy of vp_k_stft_pv_stretch_lock that marks what differs; and vp_k_stft_pv_stretch_lock and its parents are still there under
their names with the register figures their own resource tests print on the parent commit."""
import ctypes as C
import difflib
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("vp_k_stft_onset_flux", "vp_k_stft_pv_stretch_lock_reset")
# registers of the parents as their resource tests print them on the parent commit (vgpr, agpr)
PARENT_FIGURES = {"vp_k_stft_pv_stretch_lock": (361, 105), "vp_k_stft_pv_lock": (361, 105), "vp_k_stft_pv_stretch": (346, 90), "vp_k_stft_pv_curve": (346, 90),
                  "vp_k_stft_fused<true, false>": (341, 85)}
LDS_CEILING = 160 * 1024 - 512
CSRC = os.path.join(ROOT, "vocoderproject_amd", "csrc")


@pytest.fixture(scope="module")
def resources():
    from vocoderproject_amd import build
    import kernel_resources
    if not os.path.exists(os.path.join(kernel_resources.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    return kernel_resources.kernel_resources(build.build())


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_kernels_are_built_without_scratch_within_512_registers(resources, kernel):
    assert kernel in resources, sorted(k for k in resources if "stft" in k)
    r = resources[kernel]
    print(f"PV TRANSIENT resources {kernel} {r}")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 512, r
    assert r["lds"] == 0, r                                    # no static LDS: everything is the dynamic carve


def test_the_parents_keep_their_register_figures(resources):
    for parent, want in PARENT_FIGURES.items():
        assert parent in resources and resources[parent]["scratch"] == 0, (parent, resources.get(parent))
        print(f"PV TRANSIENT resources parent {parent} {resources[parent]}")
        assert (resources[parent]["vgpr"], resources[parent]["agpr"]) == want, (parent, resources[parent])


def _kernel_text(src, name):
    a = src.index(f"void {name}(")
    return src[src.index("\n", a) + 1:src.index("\n}\n", a) + 3]                      # (the body: the signature is asserted apart)


def test_the_reset_kernel_is_a_marked_copy_in_a_file_of_its_own():
    src = open(os.path.join(CSRC, "vp_stft.hip")).read()
    incs = re.findall(r'^#include "(vp_(?:stft|pv)_[a-z_]+\.inc)"', src, re.M)
    assert incs.index("vp_stft_stretch_lock.inc") < incs.index("vp_pv_transient.inc")    # behind the locked stretch, whose plan the copy uses
    assert [i for i in incs if i != "vp_pv_transient.inc"] == ["vp_stft_curve.inc", "vp_stft_stretch.inc", "vp_stft_lock.inc", "vp_stft_stretch_lock.inc", "vp_stft_cross.inc",
                                                                "vp_stft_formant.inc"]     # (the others as they were, the file still ends with the formant part)
    part = open(os.path.join(CSRC, "vp_pv_transient.inc")).read()
    assert re.findall(r'^#include "([^"]+)"', part, re.M) == ["vp_stft_onset.inc", "vp_stft_stretch_reset.inc"]
    inc = open(os.path.join(CSRC, "vp_stft_stretch_reset.inc")).read()
    assert "void vp_k_stft_pv_stretch_lock_reset(VpStftArgs A, const double *ratioTab, const int *posTab, int nIn, const unsigned char *resetTab)" in inc
    assert inc.count("#ifdef VP_POISON_LDS") == 1
    assert inc.count("reset:") >= 8
    assert "atomic" not in inc.lower()
    for helper in ("pv_lock_turn(", "pv_lock_gather(", "pv_lock_carve(", "pv_stretch_frame(", "pv_stretch_lock_plan("):
        assert helper in inc, helper
    assert "bool pv_stretch_lock_plan(" not in inc and "void pv_lock_turn(" not in inc     # used as they are, not copied
    assert "vp_k_stft_pv_stretch_lock_reset, grid, block, vp_stft_lock_lds_bytes(a.hop)" in inc
    assert "const dim3 grid(1, nStreams), block(64 * NWV);" in inc
    assert inc.count("hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512") == 1
    # statement for statement: every line of the copy that is not in the parent's kernel carries the mark, or only dropped the parent's
    # own "stretch:" mark from its comment; the parent loses no statement
    parent = _kernel_text(open(os.path.join(CSRC, "vp_stft_stretch_lock.inc")).read(), "vp_k_stft_pv_stretch_lock")
    copy = _kernel_text(inc, "vp_k_stft_pv_stretch_lock_reset")

    def code(line):
        return re.sub(r"\s+", " ", line.split("//")[0]).strip()
    pl, cl = parent.split("\n"), copy.split("\n")
    unmarked_new, lost = [], []
    for tag, a0, a1, b0, b1 in difflib.SequenceMatcher(None, [code(x) for x in pl], [code(x) for x in cl], autojunk=False).get_opcodes():
        if tag in ("replace", "insert"):
            unmarked_new += [x for x in cl[b0:b1] if code(x) and "reset:" not in x]
        if tag in ("replace", "delete"):
            lost += [x for x in pl[a0:a1] if code(x)]
    # (a replaced parent line comes back marked: the signature, the request's comment, the turn)
    assert not unmarked_new, unmarked_new
    assert len(lost) <= 3, lost
    assert open(os.path.join(CSRC, "vp_stft_stretch_lock.inc")).read().count("#ifdef VP_POISON_LDS") == 1
    capi = open(os.path.join(CSRC, "vp_capi.hip")).read()
    assert "vp_stft_onset_prepare_device() == hipSuccess && vp_stft_stretch_reset_prepare_device() == hipSuccess" in capi
    from vocoderproject_amd import build
    assert {"vp_pv_transient.inc", "vp_stft_onset.inc", "vp_stft_stretch_reset.inc", "vp_onset_host.inc"} <= set(build.DEPS)
    txt = open(os.path.join(ROOT, "vocoderproject_amd", "build.py")).read()
    assert re.search(r'"vp_stft\.hip": \[[^\]]*"vp_pv_transient\.inc", "vp_stft_onset\.inc", "vp_stft_stretch_reset\.inc"', txt)


def test_the_flux_kernel_is_a_file_of_its_own_with_the_poison_prologue():
    inc = open(os.path.join(CSRC, "vp_stft_onset.inc")).read()
    assert "void vp_k_stft_onset_flux(VpStftArgs A, int nIn, int nG, int chunk, double *flux, double *mass)" in inc
    assert inc.count("#ifdef VP_POISON_LDS") == 1
    assert inc.count("hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512") == 1
    assert "atomic" not in inc.lower() and "asm" not in inc.lower()      # plain C++: fixed-order sums, ordinary vector stores
    for used in ("fft512_rx(", "rfft_split(", "stft_load_frame(", "A.win", "A.tws", "fft_lane_init("):
        assert used in inc, used


def test_the_dynamic_lds_fits_the_ceiling_at_every_hop():
    from vocoderproject_amd import build
    lib = C.CDLL(build.build())
    one = getattr(lib, "_Z22vp_stft_lock_lds_bytesi")          # size_t vp_stft_lock_lds_bytes(int hop): the reset kernel's
    one.restype, one.argtypes = C.c_size_t, [C.c_int]
    sizes = {hop: one(hop) for hop in (64, 128, 256, 512)}
    flux = getattr(lib, "_Z23vp_stft_onset_lds_bytesv")         # size_t vp_stft_onset_lds_bytes(): the same at every hop
    flux.restype = C.c_size_t
    print(f"PV TRANSIENT dynamic LDS reset {sizes} flux {flux()}")
    for hop, b in sizes.items():
        assert 4 * 8192 < b <= LDS_CEILING, (hop, b)
    assert 4 * 8192 + 5 * 513 * 8 == flux() <= LDS_CEILING
