/*
 * emu_lazy.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * The segmented parser (zsc_amd/csrc/lz_parse_seg.h) in the lane emulation, as tests/emu builds it (whose
 * driver is included whole), with counters on what the lazy searches that cannot win cost: built once with
 * the pre-filter of the lane-parallel search and the empty-chain test on (-DSG_LAZY_FILTER=1 -DSG_EMPTY_SKIP=1)
 * and once with both off.
 *
 * g_lazy_cnt: [0] passes of the lane-parallel search entered with best >= 4, [1] passes ended after the first
 * compare, [2] compare steps, [3] passes that reach their first compare step.  The driver's own g_sg_cnt has
 * [5] searches, [12] passes, [1] long compares, [9] searches the empty-chain test skipped.
 */
extern "C" { unsigned long long g_lazy_cnt[4]; }
#define SG_LAZY_COUNT(what, n) (g_lazy_cnt[what] += (n))
#include "../emu/emu_pipeline.cpp"

extern "C" void emu_lazy_reset(void)
{
    memset(g_lazy_cnt, 0, sizeof g_lazy_cnt);
    memset(g_sg_cnt, 0, sizeof g_sg_cnt);
}
