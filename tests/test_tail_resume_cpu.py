"""Source-level checks of the tail pass's resume switch (in the manner of tests/test_shade_fixed_lists_cpu.py).

DRT_TAIL_RESUME=0 must travel as a null tail_resume pointer in the two kernels' parameter structs: read once when the context is
created, no getenv per launch and no second set of instantiations; and the resume array lives and dies with the staging array it is
indexed like."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHER = open(os.path.join(REPO, "daily-ray-trace_amd", "csrc", "drt_launcher.hip")).read()
KERNELS = open(os.path.join(REPO, "daily-ray-trace_amd", "csrc", "drt_kernels.h")).read()


def test_the_switch_is_read_once_at_context_creation():
    assert LAUNCHER.count('getenv("DRT_TAIL_RESUME")') == 1
    assert 'DRT_TAIL_RESUME' not in KERNELS
    beside = LAUNCHER.index('getenv("DRT_TRACE_TAIL")')
    assert abs(LAUNCHER.index('getenv("DRT_TAIL_RESUME")') - beside) < 1000, "read beside DRT_TRACE_TAIL, where the scene is uploaded"
    # the two places that build the kernels' parameters read the context, not the environment
    for head in ("TraceParams tp{};", "ShadeParams sp{};"):
        assert LAUNCHER.count(head) == 1
    assert len(re.findall(r"\btp\.tail_resume\s*=", LAUNCHER)) == 1 and len(re.findall(r"\bsp\.tail_resume\s*=", LAUNCHER)) == 1


def test_the_pointer_is_a_field_of_both_parameter_structs():
    trace = KERNELS[KERNELS.index("struct TraceParams"):KERNELS.index("struct WavePool")]
    shade = KERNELS[KERNELS.index("struct ShadeParams"):KERNELS.index("struct ShadeConst")]
    assert re.search(r"double\s*\*\s*tail_resume;", trace)
    assert re.search(r"const double\s*\*\s*tail_resume;", shade)
    # one set of instantiations: the template parameters of the two kernels are what they were
    assert "template <bool SCENE_IN_LDS, bool TAIL, bool LIST, bool RAYS>\n__device__ __forceinline__ void trace_paths" in KERNELS
    assert "template <bool SPDS_IN_LDS, bool XYZ, bool SIMPLE, bool LIST = false>\n__device__ __forceinline__ void shade_tail_group" in KERNELS


def test_the_resume_array_is_allocated_and_freed_with_the_staging_array():
    alloc_stage = LAUNCHER.index("ctx->d_tail_stage.need(")
    alloc_resume = LAUNCHER.index("ctx->d_tail_resume.need(")
    assert LAUNCHER.count("ctx->d_tail_resume.need(") == 1 and "ctx->d_tail_resume.remake(" not in LAUNCHER
    assert 0 < alloc_resume - alloc_stage < 300, "allocated on the line after d_tail_stage"
    line = LAUNCHER[alloc_resume - 120:LAUNCHER.index("\n", alloc_resume)]
    assert "ctx->tail_resume" in line and "npx * batch * ctx->tail_count)" in line  # in doubles, as d_tail_stage
    # both are owning members of the context (csrc/drt_owned.h), declared one after the other: freed with it, by nothing else
    context = LAUNCHER[LAUNCHER.index("struct drt_context\n"):LAUNCHER.index("static size_t trace_lds_bytes")]
    own_stage = context.index("DevBuf<double> d_tail_stage;")
    own_resume = context.index("DevBuf<double> d_tail_resume;")
    assert 0 < own_resume - own_stage < 200, "declared on the line after d_tail_stage"
    assert "hipFree(ctx->" not in LAUNCHER and "d_tail_resume.reset(" not in LAUNCHER and "d_tail_resume.release(" not in LAUNCHER
    # only contexts whose trace kernel carries tails and leaves paths to the tail pass get one, and the memory-fit check counts it
    assert re.search(r"ctx->tail_resume\s*=\s*ctx->trace_tail\s*&&\s*!ctx->tail_all_staged\s*&&", LAUNCHER)
    fixed = LAUNCHER[LAUNCHER.index("const size_t per_path_fixed"):]
    assert "ctx->tail_resume ? 2 : 1" in fixed[:fixed.index(";")]


def test_the_term_byte_keeps_its_readers():
    """the resume vertex shares the header's term byte: the mask every reader applies leaves 0 or 1"""
    mask = int(re.search(r"#define HDR_TERM_MASK (0x[0-9A-Fa-f]+)u", KERNELS).group(1), 16)
    shift = int(re.search(r"#define HDR_TERM_RESUME_SHIFT (\d+)u", KERNELS).group(1))
    field = int(re.search(r"#define HDR_TERM_RESUME_MASK (0x[0-9A-Fa-f]+)u", KERNELS).group(1), 16)
    staged = int(re.search(r"#define HDR_TERM_TAIL_STAGED (0x[0-9A-Fa-f]+)u", KERNELS).group(1), 16)
    not_done = int(re.search(r"#define HDR_TERM_NOT_DONE (0x[0-9A-Fa-f]+)u", KERNELS).group(1), 16)
    assert mask & 1 and field == 15
    parts = (mask, field << shift, staged, not_done)
    assert sum(parts) == 0xFF and all(a & b == 0 for i, a in enumerate(parts) for b in parts[i + 1:])
