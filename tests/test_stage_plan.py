"""The staging layout planner (csrc/orbx_stage.h) alone, on the CPU: a small program with its own main is compiled with g++ against the
header (no HIP) and run.  It checks the offset rules and replays two layouts of the library as literal numbers worked out from the
256-byte padding by hand: orbx_is_in_frustum's inputs and results, and the essential graph's inputs."""
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "self_commit_orb-slam2_amd" / "csrc"

PROGRAM = r"""
#include "orbx_stage.h"
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

// orbx_is_in_frustum at n points: tcw[16] | pos[3n] | normal[3n] | max[n] | min[n] | count;  x | y | xr | cos | level | in_view
static void frustum(OrbxInPlan &in, OrbxOutPlan &out, size_t n, size_t *io, size_t *oo)
{
    static const float f[1024] = {};
    static const int32_t c = 0;
    in.reset(); out.reset();
    io[0] = in.add(f, 16).off; io[1] = in.add(f, n * 3).off; io[2] = in.add(f, n * 3).off; io[3] = in.add(f, n).off; io[4] = in.add(f, n).off; io[5] = in.add(&c, 1).off;
    io[6] = in.total();
    oo[0] = out.hole<float>(n).off; oo[1] = out.hole<float>(n).off; oo[2] = out.hole<float>(n).off; oo[3] = out.hole<float>(n).off; oo[4] = out.hole<int32_t>(n).off;
    oo[5] = out.hole<uint8_t>(n).off; oo[6] = out.total();
}

int main()
{
    OrbxInPlan p;
    const uint8_t bytes[300] = {1, 2, 3};
    // counts 0, 1, 255 / 256 / 257 bytes
    CHECK(p.add(bytes, 0).off == 0 && p.total() == 0 && p.items.empty());      // room 0: nothing added, nothing moves
    CHECK(p.add(bytes, 1).off == 0 && p.total() == 256);
    CHECK(p.add(bytes, 255).off == 256 && p.total() == 512);
    CHECK(p.add(bytes, 256).off == 512 && p.total() == 768);
    CHECK(p.add(bytes, 257).off == 768 && p.total() == 1280);
    CHECK(p.add((const uint8_t *)nullptr, 0).off == 1280 && p.total() == 1280 && p.items.size() == 4);      // an absent optional array
    // room > count: 3 elements on the host, room for 100 doubles
    const double d[3] = {1.5, 2.5, 3.5};
    const auto sd = p.add(d, 3, 100);
    CHECK(sd.off == 1280 && p.total() == 1280 + 1024 && p.items.back().copy == 24 && p.items.back().room == 800);
    // a hole
    const auto sh = p.hole<int32_t>(65);
    CHECK(sh.off == 2304 && p.total() == 2304 + 512 && p.items.back().copy == 0 && p.items.back().src == nullptr);
    const auto sn = p.add((const float *)nullptr, 7);      // NULL source with a count: a hole too
    CHECK(sn.off == 2816 && p.items.back().copy == 0 && p.total() == 3072);
    CHECK(p.add(bytes, 9, 4).off == 3072 && p.items.back().copy == 4 && p.total() == 3328);      // a count above the room never copies past the room
    CHECK(p.total() % 256 == 0);
    // fill + in(): copies land at their offsets, nothing else is written (an OrbxStaged view is made by begin() alone: not here)
    std::vector<uint8_t> host(p.total(), 0xee), dev(p.total(), 0);
    p.fill(host.data());
    CHECK(sd.in(host.data())[0] == 1.5 && sd.in(host.data())[2] == 3.5 && host[1280 + 24] == 0xee);
    CHECK(host[0] == 1 && host[256] == 1 && host[256 + 255] == 0xee && host[768 + 256] == 0 && host[768 + 257] == 0xee);
    CHECK((uint8_t *)sh.in(host.data()) == host.data() + 2304 && (const uint8_t *)sh.in((const uint8_t *)dev.data()) == dev.data() + 2304);
    CHECK(host[2304] == 0xee);      // the hole is the caller's to fill
    OrbxOutPlan q;
    const auto r0 = q.hole<float>(3);
    const auto r1 = q.hole<uint8_t>(1);
    CHECK(r0.off == 0 && r1.off == 256 && q.total() == 512);
    CHECK((uint8_t *)r1.in(dev.data()) == dev.data() + 256);
    // reuse after reset: the same offsets, no new allocation
    const size_t capBefore = p.items.capacity();
    p.reset();
    CHECK(p.total() == 0 && p.items.empty());
    p.add(bytes, 1); p.add(bytes, 255); p.add(bytes, 256);
    CHECK(p.add(bytes, 257).off == 768 && p.total() == 1280 && p.items.capacity() == capBefore);
    // 1000 items: no fixed limit
    p.reset();
    size_t want = 0;
    bool okAll = true;
    for (int i = 0; i < 1000; i++) {
        okAll = okAll && p.add(bytes, (size_t)(i % 300) + 1).off == want;
        want += ((size_t)(i % 300) + 1 + 255) / 256 * 256;
    }
    CHECK(okAll && p.items.size() == 1000 && p.total() == want && p.total() % 256 == 0);

    // orbx_is_in_frustum, n = 1 and n = 65 (n * 4 = 260 bytes: one byte row more than a 256-byte unit)
    OrbxOutPlan o;
    size_t io[7], oo[7];
    frustum(p, o, 1, io, oo);
    const size_t in1[7] = {0, 256, 512, 768, 1024, 1280, 1536}, out1[7] = {0, 256, 512, 768, 1024, 1280, 1536};
    for (int i = 0; i < 7; i++) CHECK(io[i] == in1[i] && oo[i] == out1[i]);
    frustum(p, o, 65, io, oo);
    const size_t in65[7] = {0, 256, 1280, 2304, 2816, 3328, 3584}, out65[7] = {0, 512, 1024, 1536, 2048, 2560, 2816};
    for (int i = 0; i < 7; i++) CHECK(io[i] == in65[i] && oo[i] == out65[i]);

    // the essential graph's inputs at N = 2 vertices, E = 1 edge, M = 0 points (one free vertex: nf = 1, nOff = 0, one assembly item):
    // est[8N] | meas[8N] | at[8N] doubles, edges[3E], points[3M] floats, ref[M], pos[N], colPtr[nf + 1], rowIdx[nOff], aPtr[nf + nOff + 1], aItem
    const double est[16] = {};
    const int32_t idx[8] = {};
    const float pts[1] = {};
    const size_t N = 2, E = 1, M = 0, nf = 1, nOff = 0, nA = 1;
    p.reset();
    const size_t eg[12] = {p.add(est, 8 * N).off, p.add(est, 8 * N).off, p.add(est, 8 * N).off, p.add(idx, 3 * E).off, p.add(pts, 3 * M).off, p.add(idx, M).off, p.add(idx, N).off,
                           p.add(idx, nf + 1).off, p.add(idx, nOff).off, p.add(idx, nf + nOff + 1).off, p.add(idx, nA).off, p.total()};
    const size_t egWant[12] = {0, 256, 512, 768, 1024, 1024, 1024, 1280, 1536, 1536, 1792, 2048};
    for (int i = 0; i < 12; i++) CHECK(eg[i] == egWant[i]);
    CHECK(p.items.size() == 8);      // the three empty arrays took no item

    if (failures) printf("%d checks failed\n", failures);
    else printf("all checks passed\n");
    return failures ? 1 : 0;
}
"""


def test_stage_plan_program():
    with tempfile.TemporaryDirectory() as d:
        src, exe = Path(d) / "stage_plan.cc", Path(d) / "stage_plan"
        src.write_text(PROGRAM)
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + str(CSRC), "-o", str(exe), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "all checks passed", r.stdout


def test_stage_header_is_host_only():
    text = (CSRC / "orbx_stage.h").read_text()
    assert "#include <hip" not in text and '#include "orbx_' not in text, "orbx_stage.h must compile without HIP and without the library's other headers"
