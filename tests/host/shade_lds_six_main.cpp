/* Host program of tests/test_closed_shade_six_waves_resources.py: the LDS rule's six-wave shape (csrc/drt_shade_lds_rule.h,
 * shade_lds_plan_six), run as the launcher runs it.
 *
 * stdin:  lines `n_spd S spds_in_lds wave_words`
 * stdout: per line `table_bytes wave_bytes group_bytes granted_bytes groups_by_lds groups waves_per_simd fits` */
#include <cstdio>

#include "drt_shade_lds_rule.h"

int main()
{
    unsigned n_spd, S, in_lds, wave_words;
    while (scanf("%u %u %u %u", &n_spd, &S, &in_lds, &wave_words) == 4)
    {
        const ShadeLdsPlan p = shade_lds_plan_six(n_spd, S, in_lds != 0, wave_words);
        printf("%zu %zu %zu %zu %u %u %u %d\n", p.table_bytes, p.wave_bytes, p.group_bytes, p.granted_bytes, p.groups_by_lds, p.groups, p.waves_per_simd,
               shade_lds_six_fits(p) ? 1 : 0);
    }
    return 0;
}
