"""The packing stage of k_pyr_band's resize blend (csrc/orbx_pack.h: four blend sums -> the four bytes of an output word) on the CPU: a small
program with its own main is compiled with g++ against the header (no HIP) and runs EVERY pair of sums in 0 .. 1023 through both halves of the
packed path - as pixels 0 and 1 (the low operand of the byte permute) and as pixels 2 and 3 (the high one) - against ((m + 2) >> 2) & 255 per pixel.
The blend's sums are at most 1020; the pairs above that show that a lane's carry into its high byte never reaches a neighbouring pixel."""
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "self_commit_orb-slam2_amd" / "csrc"

PROGRAM = r"""
#include "orbx_pack.h"
#include <cstdio>

static long failures = 0, checked = 0;
static uint32_t want(uint32_t m) { return ((m + 2u) >> 2) & 255u; }

static void check(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3)
{
    const uint32_t got = orbx_pack4_round_shr2(m0, m1, m2, m3), exp = want(m0) | (want(m1) << 8) | (want(m2) << 16) | (want(m3) << 24);
    checked++;
    if (got != exp && failures++ < 10) printf("pack(%u, %u, %u, %u): want %08x, got %08x\n", m0, m1, m2, m3, exp, got);
}

int main()
{
    // the other half holds a fixed pattern that differs from pair to pair, so that a byte taken from the wrong half shows
    for (uint32_t a = 0; a < 1024; a++)
        for (uint32_t b = 0; b < 1024; b++) {
            const uint32_t c = (a * 7u + b * 13u + 5u) & 1023u, d = (a * 3u + b * 11u + 1021u) & 1023u;
            check(a, b, c, d);      // the pair as pixels 0, 1
            check(c, d, a, b);      // the pair as pixels 2, 3
        }
    // the two stages on their own: 16-bit lanes, and the permute's byte order
    if (orbx_pack2_round_shr2(1021u, 2u) != ((1u << 16) | 255u)) { failures++; printf("pack2 lanes\n"); }
    if (orbx_byte_perm(0x77665544u, 0x33221100u, 0x06040200u) != 0x66442200u) { failures++; printf("byte permute\n"); }
    printf("%ld checked, %ld failed\n", checked, failures);
    return failures ? 1 : 0;
}
"""


def test_packed_blend_equals_the_per_pixel_form_for_every_pair_of_sums():
    with tempfile.TemporaryDirectory() as d:
        src, exe = Path(d) / "pack.cc", Path(d) / "pack"
        src.write_text(PROGRAM)
        r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I" + str(CSRC), "-o", str(exe), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(" 0 failed") and int(r.stdout.split()[0]) == 2 * 1024 * 1024, r.stdout


def test_pack_header_is_host_compilable_and_the_kernel_uses_it():
    text = (CSRC / "orbx_pack.h").read_text()
    assert "#include <hip" not in text and '#include "orbx_' not in text, "orbx_pack.h must compile without HIP and without the library's other headers"
    kernels = (CSRC / "orbx_kernels.hip").read_text()
    assert '#include "orbx_pack.h"' in kernels and "orbx_pack4_round_shr2(" in kernels
