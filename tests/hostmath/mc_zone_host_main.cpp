// TEST-ONLY stand-alone program around tests/hostmath/mc_zone_host.cpp, for a sanitizer build of the zone engine's host twin (a sanitizer
// does not see code loaded into Python): g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined mc_zone_host_main.cpp -o
// mc_zone_host_main, then mc_zone_host_main SCENE...  A scene file is what tests/mc_zone_ref.dump writes: int32 nx, transition, nComp, T,
// nZone, nVert, K, S; uint64 seed; float64 dt, 0; then Phi [nx][nx], Q [nx][nx], x [nx][nComp], P [nx (nx + 1) / 2][nComp], cdf [nComp]
// and zoneXY [nVert][2] in float64, first [T + 1] and zoneFirst [nZone + 1] in int32.  Prints the sums of the counts; exit status 1 for a
// file it cannot read or a call the twin refuses.
#include "mc_zone_host.cpp"

#include <cstdio>

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 1;
        int32_t h[8];
        uint64_t seed;
        double dr[2];
        if (!read_all(f, h, sizeof h) || !read_all(f, &seed, sizeof seed) || !read_all(f, dr, sizeof dr) || h[0] < 1 || h[0] > 6 || h[2] < 1 || h[3] < 1 || h[4] < 1 ||
            h[4] > MC_ZONE_MAX_ZONES || h[5] < 1 || h[5] > MC_ZONE_MAX_VERTS || h[6] < 1 || h[6] > MC_MAX_STEPS) {
            fclose(f);
            return 1;
        }
        const size_t nx = (size_t)h[0], n = (size_t)h[2], T = (size_t)h[3], nZ = (size_t)h[4], nV = (size_t)h[5], K1 = (size_t)h[6] + 1;
        std::vector<double> Phi(nx * nx), Q(nx * nx), x(nx * n), P(nx * (nx + 1) / 2 * n), cdf(n), xy(nV * 2);
        std::vector<int32_t> first(T + 1), zoneFirst(nZ + 1), status(T);
        std::vector<uint32_t> inside(nZ * K1 * T), firstAt(nZ * K1 * T), ever(nZ * T), valid(T);
        bool ok = true;
        for (std::vector<double>* v : {&Phi, &Q, &x, &P, &cdf, &xy}) ok = ok && read_all(f, v->data(), v->size() * sizeof(double));
        ok = ok && read_all(f, first.data(), first.size() * sizeof(int32_t)) && read_all(f, zoneFirst.data(), zoneFirst.size() * sizeof(int32_t));
        fclose(f);
        if (!ok) return 1;
        if (mc_zone_encounters_host(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], seed, dr[0], Phi.data(), Q.data(), x.data(), P.data(), first.data(), cdf.data(),
                                    zoneFirst.data(), xy.data(), inside.data(), firstAt.data(), ever.data(), valid.data(), status.data()) != 0)
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
