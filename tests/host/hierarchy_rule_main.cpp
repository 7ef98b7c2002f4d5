/*
 * The hierarchy rule's own text (csrc/drt_build_rule.h) on the host: tests/test_hierarchy_cpu.py builds this with the address and
 * undefined-behaviour sanitizers and compares what it prints with tests/hierarchy_rule.py. The kernels compile the same header.
 *
 * stdin:  m, then m lines "bounded cx cy cz": whether the box of tree position k is bounded, and its centre (hexadecimal doubles);
 *         or the word "keys", m, then m keys in decimal: the keys themselves, for key sets no scene gives (tests/build_pass_cases.py)
 * stdout: "levels L", then "key k" per position, "slot position" per leaf slot in order, "node child0 child1 count0 count1" per node
 */
#include "drt_build_rule.h"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

int main()
{
    uint32_t m = 0;
    char word[32];
    if (scanf("%31s", word) != 1) return 2;
    const bool raw = strcmp(word, "keys") == 0;
    if ((raw ? scanf("%" SCNu32, &m) : sscanf(word, "%" SCNu32, &m)) != 1) return 2;
    std::vector<uint64_t> key(m);
    std::vector<double> c(3 * (size_t)m);
    std::vector<uint32_t> bounded(m);
    double clo[3] = {0.0, 0.0, 0.0}, chi[3] = {0.0, 0.0, 0.0};
    bool any = false;
    for (uint32_t k = 0; raw && k < m; k += 1)
        if (scanf("%" SCNu64, &key[k]) != 1 || key[k] > BUILD_KEY_UNBOUNDED) return 2;
    for (uint32_t k = 0; !raw && k < m; k += 1)
    {
        if (scanf("%" SCNu32 " %la %la %la", &bounded[k], &c[3 * k], &c[3 * k + 1], &c[3 * k + 2]) != 4) return 2;
        if (!bounded[k]) continue;
        for (int a = 0; a < 3; a += 1)
        {
            const double x = c[3 * k + a];
            clo[a] = !any || x < clo[a] ? x : clo[a];
            chi[a] = !any || chi[a] < x ? x : chi[a];
        }
        any = true;
    }
    for (uint32_t k = 0; !raw && k < m; k += 1)
        key[k] = bounded[k] ? build_key(build_quantise(c[3 * k], clo[0], chi[0]), build_quantise(c[3 * k + 1], clo[1], chi[1]), build_quantise(c[3 * k + 2], clo[2], chi[2]))
                            : BUILD_KEY_UNBOUNDED;
    std::vector<uint32_t> order(m);
    for (uint32_t k = 0; k < m; k += 1) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    std::vector<uint64_t> sorted(m);
    for (uint32_t j = 0; j < m; j += 1) sorted[j] = key[order[j]];
    const uint32_t n = m > 1 ? m - 1 : 1;
    std::vector<int32_t> child(2 * (size_t)n), count(2 * (size_t)n);
    const uint32_t levels = build_topology_serial(sorted.data(), m, child.data(), count.data());
    printf("levels %" PRIu32 "\n", levels);
    for (uint32_t k = 0; k < m; k += 1) printf("key %" PRIu64 "\n", key[k]);
    for (uint32_t j = 0; j < m; j += 1) printf("slot %" PRIu32 "\n", order[j]);
    for (uint32_t i = 0; i < n; i += 1) printf("node %d %d %d %d\n", child[2 * i], child[2 * i + 1], count[2 * i], count[2 * i + 1]);
    return 0;
}
