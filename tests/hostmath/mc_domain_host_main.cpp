// TEST-ONLY stand-alone program around tests/hostmath/mc_domain_host.cpp, for a sanitizer build of the domain engine's host twin (a
// sanitizer does not see code loaded into Python): g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined
// mc_domain_host_main.cpp -o mc_domain_host_main, then mc_domain_host_main SCENE...  A scene file is what tests/mc_domain_ref.dump
// writes: int32 nx, transition, nComp, T, G, nDomain, nVert, K, S, 0; uint64 seed; float64 dt, 0; then Phi [nx][nx], Q [nx][nx],
// x [nx][nComp], P [nx (nx + 1) / 2][nComp], cdf [nComp], domXY [nVert][2] and ownPose [G][K + 1][4] in float64, first [T + 1] and
// domFirst [nDomain + 1] in int32.  Prints the sums of the counts; exit status 1 for a file it cannot read or a call the twin refuses.
#include "mc_domain_host.cpp"

#include <cstdio>

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 1;
        int32_t h[10];
        uint64_t seed;
        double dr[2];
        if (!read_all(f, h, sizeof h) || !read_all(f, &seed, sizeof seed) || !read_all(f, dr, sizeof dr) || h[0] < 1 || h[0] > 6 || h[2] < 1 || h[3] < 1 || h[4] < 1 ||
            h[4] > MC_DOMAIN_MAX_CELLS || h[5] < 1 || h[5] > MC_DOMAIN_MAX_DOMAINS || h[6] < 1 || h[6] > MC_DOMAIN_MAX_VERTS || h[7] < 1 || h[7] > MC_MAX_STEPS) {
            fclose(f);
            return 1;
        }
        const size_t nx = (size_t)h[0], n = (size_t)h[2], T = (size_t)h[3], G = (size_t)h[4], nD = (size_t)h[5], nV = (size_t)h[6], K1 = (size_t)h[7] + 1;
        std::vector<double> Phi(nx * nx), Q(nx * nx), x(nx * n), P(nx * (nx + 1) / 2 * n), cdf(n), xy(nV * 2), pose(G * K1 * 4);
        std::vector<int32_t> first(T + 1), domFirst(nD + 1), status(T);
        std::vector<uint32_t> inside(nD * G * K1 * T), firstAt(nD * G * K1 * T), ever(nD * G * T), valid(T);
        bool ok = true;
        for (std::vector<double>* v : {&Phi, &Q, &x, &P, &cdf, &xy, &pose}) ok = ok && read_all(f, v->data(), v->size() * sizeof(double));
        ok = ok && read_all(f, first.data(), first.size() * sizeof(int32_t)) && read_all(f, domFirst.data(), domFirst.size() * sizeof(int32_t));
        fclose(f);
        if (!ok) return 1;
        if (mc_domain_encounters_host(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], seed, dr[0], Phi.data(), Q.data(), x.data(), P.data(), first.data(),
                                      cdf.data(), pose.data(), domFirst.data(), xy.data(), 1, inside.data(), firstAt.data(), ever.data(), valid.data(),
                                      status.data()) != 0)
            return 1;
        unsigned long long si = 0, sf = 0, se = 0, sv = 0;
        for (uint32_t v : inside) si += v;
        for (uint32_t v : firstAt) sf += v;
        for (uint32_t v : ever) se += v;
        for (uint32_t v : valid) sv += v;
        printf("%s: inside %llu firstAt %llu ever %llu valid %llu\n", argv[a], si, sf, se, sv);
    }
    return 0;
}
