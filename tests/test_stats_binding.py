"""CPU checks of the lease-statistics binding: the tile and slot counts the binding states
(tests/test_gpu_stats.py sizes its cases by them) are the kernel's own, and the flag is the
header's."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_states_the_kernel_shape():
    from distributedratelimiting.redis_amd import _capi
    src = open(os.path.join(ROOT, "distributedratelimiting.redis_amd", "csrc", "tbe_stats.hpp")).read()
    tile = int(re.search(r"constexpr int kStatsTile = (\d+);", src).group(1))
    bits = int(re.search(r"constexpr uint32_t kStatsSlotBits = (\d+);", src).group(1))
    assert (_capi.STATS_TILE, _capi.STATS_SLOTS) == (tile, 1 << bits)


def test_flag_matches_the_header():
    from distributedratelimiting.redis_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "tbe.h")).read()
    assert int(re.search(r"#define TBE_FLAG_STATS (0x[0-9a-fA-F]+)u", hdr).group(1), 16) == _capi.TBE_FLAG_STATS == 0x200
    others = [int(x, 16) for x in re.findall(r"#define TBE_FLAG_(?!STATS)\w+ (0x[0-9a-fA-F]+)u", hdr)]
    assert all(o & 0x200 == 0 for o in others)
