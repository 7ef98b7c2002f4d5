/* Host program of tests/test_closed_shade_resources.py: the shade kernels' LDS rule (csrc/drt_shade_lds_rule.h), run as the launcher
 * runs it.
 *
 * stdin:  lines `n_spd S spds_in_lds block_waves wave_words register_waves`
 * stdout: per line `table_bytes wave_bytes group_bytes granted_bytes groups_by_lds groups waves_per_simd` */
#include <cstdio>

#include "drt_shade_lds_rule.h"

int main()
{
    unsigned n_spd, S, in_lds, block_waves, wave_words, register_waves;
    while (scanf("%u %u %u %u %u %u", &n_spd, &S, &in_lds, &block_waves, &wave_words, &register_waves) == 6)
    {
        const ShadeLdsPlan p = shade_lds_plan(n_spd, S, in_lds != 0, block_waves, wave_words, register_waves);
        printf("%zu %zu %zu %zu %u %u %u\n", p.table_bytes, p.wave_bytes, p.group_bytes, p.granted_bytes, p.groups_by_lds, p.groups, p.waves_per_simd);
    }
    return 0;
}
