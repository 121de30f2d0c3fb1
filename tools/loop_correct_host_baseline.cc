// tools/loop_correct_host_baseline.cc -- the host column of profiles/loop_correct_latency.txt: this project's own one-thread statement of the two
// loops that orbx_loop_correct_sim3 and orbx_loop_propagate_gba run on the device, on plain arrays (no mutexes, no cv::Mat, no std::map walks:
// all of which the reference's bodies pay for on top).  Same arithmetic, operation by operation (build with -ffp-contract=off), so the checksum of
// its results must equal the device's.
//
//   loop_correct_host_baseline scene.bin mode reps      mode 0 = CorrectLoop's Sim3 propagation, 1 = the map update after global BA
//   -> "mode  median microseconds  checksum"
// scene.bin: tools/latency_loop_correct.py writes it (a header of int32 sizes, then the arrays of the problem struct in declaration order).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

struct Sim3 { double q[4], t[3], s; };

static void quat_from_R(const double *R, double *q)
{
    double t = (R[0] + R[4]) + R[8];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
        return;
    }
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    t = std::sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0);
    q[i] = 0.5 * t; t = 0.5 / t;
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t; q[j] = (R[3 * j + i] + R[3 * i + j]) * t; q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
}
static void rotate(const double *q, const double *v, double *o)
{
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int c = 0; c < 3; c++) uv[c] = uv[c] + uv[c];
    o[0] = (v[0] + q[3] * uv[0]) + (q[1] * uv[2] - q[2] * uv[1]);
    o[1] = (v[1] + q[3] * uv[1]) + (q[2] * uv[0] - q[0] * uv[2]);
    o[2] = (v[2] + q[3] * uv[2]) + (q[0] * uv[1] - q[1] * uv[0]);
}
static void map3(const Sim3 &S, const double *v, double *o)
{
    double r[3];
    rotate(S.q, v, r);
    for (int c = 0; c < 3; c++) o[c] = S.s * r[c] + S.t[c];
}
static Sim3 mul(const Sim3 &a, const Sim3 &b)
{
    Sim3 o;
    const double *p = a.q, *r = b.q;
    o.q[3] = ((p[3] * r[3] - p[0] * r[0]) - p[1] * r[1]) - p[2] * r[2];
    o.q[0] = ((p[3] * r[0] + p[0] * r[3]) + p[1] * r[2]) - p[2] * r[1];
    o.q[1] = ((p[3] * r[1] + p[1] * r[3]) + p[2] * r[0]) - p[0] * r[2];
    o.q[2] = ((p[3] * r[2] + p[2] * r[3]) + p[0] * r[1]) - p[1] * r[0];
    double rt[3];
    rotate(a.q, b.t, rt);
    for (int c = 0; c < 3; c++) o.t[c] = a.s * rt[c] + a.t[c];
    o.s = a.s * b.s;
    return o;
}
static Sim3 inverse(const Sim3 &a)
{
    Sim3 o;
    o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
    const double f = -1.0 / a.s, v[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
    rotate(o.q, v, o.t);
    o.s = 1.0 / a.s;
    return o;
}
static void quat_to_R(const double *q, double *R)
{
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
// a pose is 3x4 float rows over 0 0 0 1
static void inverse_pose(const float *T, float *Twc)      // SetPose: Rwc = Rcw^T, Ow = (-Rwc) * tcw
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Twc[4 * i + j] = T[4 * j + i];
        Twc[4 * i + 3] = ((-Twc[4 * i]) * T[3] + (-Twc[4 * i + 1]) * T[7]) + (-Twc[4 * i + 2]) * T[11];
    }
}
static void mul44(const float *A, const float *B, float *C)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) C[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * (j == 3 ? 1.0f : 0.0f);
}
static Sim3 sim3_of_pose(const float *T)
{
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    Sim3 S;
    quat_from_R(R, S.q);
    S.t[0] = T[3]; S.t[1] = T[7]; S.t[2] = T[11]; S.s = 1.0;
    return S;
}
static double norm3(const float *v)
{
    double s = 0.0;
    for (int c = 0; c < 3; c++) s = s + (double)v[c] * (double)v[c];
    return std::sqrt(s);
}

template <typename T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short scene file\n"); exit(2); }
    return v;
}
static uint64_t bits(const float *a, size_t n)
{
    uint64_t s = 0;
    for (size_t i = 0; i < n; i++) { uint32_t u; memcpy(&u, a + i, 4); s += (uint64_t)u * (uint64_t)(i % 7 + 1); }
    return s;
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    const int mode = atoi(argv[2]), reps = atoi(argv[3]);
    if (!f) return 2;
    std::vector<int32_t> hd = take<int32_t>(f, 8);
    std::vector<double> times;
    uint64_t chk = 0;
    if (mode == 0) {
        const int NK = hd[1], G = hd[2], cur = hd[3], S = hd[4], M = hd[5], T = hd[6];
        const std::vector<float> tcw = take<float>(f, 12 * (size_t)NK), ow0 = take<float>(f, 3 * (size_t)NK);
        const std::vector<int32_t> group = take<int32_t>(f, G);
        const std::vector<double> scw = take<double>(f, 8);
        const std::vector<int32_t> loff = take<int32_t>(f, G + 1), lpt = take<int32_t>(f, S);
        const std::vector<float> pos0 = take<float>(f, 3 * (size_t)M);
        const std::vector<uint8_t> bad = take<uint8_t>(f, M), done0 = take<uint8_t>(f, M);
        const std::vector<int32_t> ref = take<int32_t>(f, M);
        const std::vector<float> rsc = take<float>(f, M), tsc = take<float>(f, M);
        const std::vector<int32_t> ooff = take<int32_t>(f, M + 1), okf = take<int32_t>(f, T);
        for (int rep = 0; rep < reps; rep++) {
            std::vector<float> ow = ow0, pos = pos0, normal(3 * (size_t)M, 0.f), mx(M, 0.f), mn(M, 0.f), tiw(12 * (size_t)G);
            std::vector<uint8_t> done = done0;
            const auto t0 = std::chrono::steady_clock::now();
            Sim3 Scw;
            memcpy(Scw.q, scw.data(), 32); memcpy(Scw.t, scw.data() + 4, 24); Scw.s = scw[7];
            float Twc[12];
            inverse_pose(&tcw[12 * (size_t)group[cur]], Twc);
            std::vector<Sim3> corr(G), nonc(G);
            for (int g = 0; g < G; g++) {
                const float *Tiw = &tcw[12 * (size_t)group[g]];
                if (g != cur) { float Tic[12]; mul44(Tiw, Twc, Tic); corr[g] = mul(sim3_of_pose(Tic), Scw); } else corr[g] = Scw;
                nonc[g] = sim3_of_pose(Tiw);
            }
            for (int g = 0; g < G; g++) {
                const Sim3 swi = inverse(corr[g]);
                for (int e = loff[g]; e < loff[g + 1]; e++) {
                    const int i = lpt[e];
                    if (i < 0 || bad[i] || done[i]) continue;
                    const double X[3] = {pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]};
                    double a[3], b[3];
                    map3(nonc[g], X, a); map3(swi, a, b);
                    float *P = &pos[3 * (size_t)i];
                    for (int c = 0; c < 3; c++) P[c] = (float)b[c];
                    done[i] = 1;
                    const int n = ooff[i + 1] - ooff[i];
                    if (!n) continue;
                    float acc[3] = {0.f, 0.f, 0.f};
                    for (int o = ooff[i]; o < ooff[i + 1]; o++) {
                        const float *O = &ow[3 * (size_t)okf[o]];
                        const float v[3] = {P[0] - O[0], P[1] - O[1], P[2] - O[2]};
                        const double s = norm3(v);
                        for (int c = 0; c < 3; c++) acc[c] = acc[c] + (float)((double)v[c] / s);
                    }
                    for (int c = 0; c < 3; c++) normal[3 * (size_t)i + c] = (float)((double)acc[c] / (double)n);
                    const float *O = &ow[3 * (size_t)ref[i]];
                    const float v[3] = {P[0] - O[0], P[1] - O[1], P[2] - O[2]};
                    const float dist = (float)norm3(v);
                    mx[i] = dist * rsc[i]; mn[i] = mx[i] / tsc[i];
                }
                double R[9];
                quat_to_R(corr[g].q, R);
                const double inv = 1.0 / corr[g].s;
                float *Tn = &tiw[12 * (size_t)g], Tw[12];
                for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Tn[4 * r + c] = (float)R[3 * r + c]; Tn[4 * r + 3] = (float)(corr[g].t[r] * inv); }
                inverse_pose(Tn, Tw);
                for (int c = 0; c < 3; c++) ow[3 * (size_t)group[g] + c] = Tw[4 * c + 3];
            }
            times.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
            chk = bits(pos.data(), pos.size()) + 3 * bits(normal.data(), normal.size()) + 5 * bits(mx.data(), mx.size()) + 7 * bits(mn.data(), mn.size()) + 11 * bits(tiw.data(), tiw.size());
        }
    } else {
        const int n = hd[1], M = hd[2];
        const std::vector<int32_t> parent = take<int32_t>(f, n);
        const std::vector<float> tcw0 = take<float>(f, 12 * (size_t)n), gba0 = take<float>(f, 12 * (size_t)n);
        const std::vector<uint8_t> in0 = take<uint8_t>(f, n);
        const std::vector<float> pos0 = take<float>(f, 3 * (size_t)M), pgba = take<float>(f, 3 * (size_t)M);
        const std::vector<uint8_t> pin = take<uint8_t>(f, M), pbad = take<uint8_t>(f, M);
        const std::vector<int32_t> pref = take<int32_t>(f, M);
        for (int rep = 0; rep < reps; rep++) {
            std::vector<float> pose = tcw0, gba = gba0, bef(12 * (size_t)n, 0.f), pos = pos0;
            std::vector<uint8_t> in = in0, reached(n, 0);
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<int32_t> coff(n + 1, 0), child(n);
            for (int i = 0; i < n; i++) if (parent[i] >= 0) coff[parent[i] + 1]++;
            for (int i = 0; i < n; i++) coff[i + 1] += coff[i];
            { std::vector<int32_t> at(coff.begin(), coff.end() - 1); for (int i = 0; i < n; i++) if (parent[i] >= 0) child[at[parent[i]]++] = i; }
            std::deque<int> todo;
            for (int i = 0; i < n; i++) if (parent[i] == -1) todo.push_back(i);
            while (!todo.empty()) {
                const int k = todo.front();
                float Twc[12];
                inverse_pose(&pose[12 * (size_t)k], Twc);
                for (int e = coff[k]; e < coff[k + 1]; e++) {
                    const int c = child[e];
                    if (!in[c]) { float Tcp[12]; mul44(&pose[12 * (size_t)c], Twc, Tcp); mul44(Tcp, &gba[12 * (size_t)k], &gba[12 * (size_t)c]); in[c] = 1; }
                    todo.push_back(c);
                }
                memcpy(&bef[12 * (size_t)k], &pose[12 * (size_t)k], 48);
                memcpy(&pose[12 * (size_t)k], &gba[12 * (size_t)k], 48);
                reached[k] = 1;
                todo.pop_front();
            }
            for (int i = 0; i < M; i++) {
                if (pbad[i]) continue;
                float *X = &pos[3 * (size_t)i];
                if (pin[i]) { memcpy(X, &pgba[3 * (size_t)i], 12); continue; }
                const int r = pref[i];
                if (r < 0 || !reached[r]) continue;
                const float *B = &bef[12 * (size_t)r];
                float Xc[3], Twc[12];
                for (int c = 0; c < 3; c++) Xc[c] = ((B[4 * c] * X[0] + B[4 * c + 1] * X[1]) + B[4 * c + 2] * X[2]) + B[4 * c + 3];
                inverse_pose(&pose[12 * (size_t)r], Twc);
                for (int c = 0; c < 3; c++) X[c] = ((Twc[4 * c] * Xc[0] + Twc[4 * c + 1] * Xc[1]) + Twc[4 * c + 2] * Xc[2]) + Twc[4 * c + 3];
            }
            times.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
            chk = bits(pos.data(), pos.size()) + 3 * bits(gba.data(), gba.size());
        }
    }
    fclose(f);
    std::sort(times.begin(), times.end());
    printf("%d %.3f %llu\n", mode, times[times.size() / 2], (unsigned long long)chk);
    return 0;
}
