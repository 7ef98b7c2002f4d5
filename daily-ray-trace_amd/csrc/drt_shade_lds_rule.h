/*
 * drt_shade_lds_rule.h -- what a shade launch asks of a compute unit's LDS, and how many of its workgroups that lets stay resident.
 *
 * Plain C++, no HIP: the launcher (drt_launcher.hip, create_impl) sizes the shade kernels' dynamic LDS from shade_lds_plan() and never
 * counts on more workgroups per compute unit than it returns; a host test calls the very same text (tests/host). The kernels' own
 * constants (SHADE_WAVES, the words of a wave's region: SHADE_WAVE_LDS_WORDS_FOR in drt_kernels.h) come in as arguments.
 *
 * A shade workgroup holds the SPD table once ([n_spd][S] doubles, where it is kept in LDS) and one region per wave behind it. A wave
 * per SIMD more needs a workgroup per compute unit more, so the register bound of an instantiation is only reached where that many
 * workgroups also fit the LDS: the headline scene's table is 38 rows of 69 (20 976 bytes), and with the 2 912-byte regions of the
 * general instantiations a workgroup is 32 624 bytes -- five of them are 163 120 bytes, inside 160 KiB only if LDS were handed out to
 * the byte. It is handed out in granules; with them four workgroups fit, whatever the registers allow.
 *
 * A sixth wave per SIMD as a sixth workgroup of four waves is out of reach for that table: 163 840 / 6 is 26 880 bytes in granules, and
 * the table alone takes 20 976. The table is the same in every workgroup, so the six-wave form has workgroups of eight waves that
 * share one copy: shade_lds_plan_six() -- 20 976 + 8 x 2 560 = 41 456 bytes, 33 granules, and three such workgroups (24 waves, six per
 * SIMD) are 126 720 bytes.
 */
#ifndef DRT_SHADE_LDS_RULE_H
#define DRT_SHADE_LDS_RULE_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

#define SHADE_LDS_PER_CU (160u * 1024u) /* gfx950 */
/* LDS is allocated to a workgroup in granules. 1280 bytes (320 dwords) is what the compiler's kernel descriptors count in on targets
 * with 160 KiB; were the hardware's granule smaller, this rule would only leave room unused. */
#define SHADE_LDS_GRANULE 1280u
#define SHADE_SIMDS_PER_CU 4u

struct ShadeLdsPlan
{
    size_t   table_bytes;   /* the SPD table's copy (0: read from memory) */
    size_t   wave_bytes;    /* a wave's own region */
    size_t   group_bytes;   /* what a launch asks for: table + waves x region */
    size_t   granted_bytes; /* ... rounded up to granules */
    uint32_t groups_by_lds; /* workgroups a compute unit's LDS holds */
    uint32_t groups;        /* ... and its registers: resident workgroups per compute unit */
    uint32_t waves_per_simd;
};

/* block_waves: waves per workgroup (a multiple of the SIMDs, so that they spread evenly); wave_words: 64-bit words of a wave's region;
 * register_waves: waves per SIMD the instantiation's register allocation allows */
static inline ShadeLdsPlan shade_lds_plan(uint32_t n_spd, uint32_t S, bool spds_in_lds, uint32_t block_waves, uint32_t wave_words, uint32_t register_waves)
{
    ShadeLdsPlan p{};
    p.table_bytes = spds_in_lds ? (size_t)n_spd * S * 8 : 0;
    p.wave_bytes = (size_t)wave_words * 8;
    p.group_bytes = p.table_bytes + (size_t)block_waves * p.wave_bytes;
    p.granted_bytes = (p.group_bytes + SHADE_LDS_GRANULE - 1) / SHADE_LDS_GRANULE * SHADE_LDS_GRANULE;
    p.groups_by_lds = p.granted_bytes ? (uint32_t)(SHADE_LDS_PER_CU / p.granted_bytes) : ~0u;
    const uint32_t groups_by_registers = register_waves * SHADE_SIMDS_PER_CU / std::max(1u, block_waves);
    p.groups = std::min(p.groups_by_lds, groups_by_registers);
    p.waves_per_simd = p.groups * block_waves / SHADE_SIMDS_PER_CU;
    return p;
}

/* The six-wave shape: workgroups of SHADE_LDS_SIX_BLOCK_WAVES waves behind one table, SHADE_LDS_SIX_GROUPS of them on a compute unit. */
#define SHADE_LDS_SIX_BLOCK_WAVES 8u
#define SHADE_LDS_SIX_WAVES_PER_SIMD 6u
#define SHADE_LDS_SIX_GROUPS (SHADE_LDS_SIX_WAVES_PER_SIMD * SHADE_SIMDS_PER_CU / SHADE_LDS_SIX_BLOCK_WAVES) /* 3 */

static inline ShadeLdsPlan shade_lds_plan_six(uint32_t n_spd, uint32_t S, bool spds_in_lds, uint32_t wave_words)
{
    return shade_lds_plan(n_spd, S, spds_in_lds, SHADE_LDS_SIX_BLOCK_WAVES, wave_words, SHADE_LDS_SIX_WAVES_PER_SIMD);
}

/* whether the shape keeps its six waves per SIMD beside this table (the launcher then still asks the runtime) */
static inline bool shade_lds_six_fits(const ShadeLdsPlan &p) { return p.groups >= SHADE_LDS_SIX_GROUPS; }

#endif
