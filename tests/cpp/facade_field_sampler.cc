// C++ drop-in test of include/MeshFEMHip/FieldSampler.hh on a quadratic tet Simulator and on a raw mesh: prints what the five methods return;
// tests/test_cpp_field_sampler.py compares the numbers with the numpy restatement (tests/field_sampler_util.py).
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), point file (f64 P[nP][3]), field file
// (f64 f[nNode][2]), output file.
// Output (all f64): I [nP], B [nP][4], C [nP][3], sqDist [nP], NI [nP], node sqDist [nP], contains [nP], sample of the nodal field [nP][2],
// I of the raw-mesh sampler [nP], its sample of the per-vertex field x + 2 y - z [nP].
#include <MeshFEMHip/FieldSampler.hh>
#include <cstdio>
#include <cstdlib>

using namespace MeshFEMHip;

static void put(FILE *f, const std::vector<Real> &v) { fwrite(v.data(), sizeof(Real), v.size(), f); }
static std::vector<Real> asReal(const std::vector<int32_t> &v) { return std::vector<Real>(v.begin(), v.end()); }

int main(int argc, char **argv) {
    const int device = argc > 1 ? atoi(argv[1]) : 0;
    std::vector<std::array<Real, 3>> V = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};      // one tetrahedron: enough to reach the device (or fail to)
    std::vector<std::array<int32_t, 4>> T = {{0, 1, 2, 3}};
    std::vector<Real> P = {0.1, 0.2, 0.3, 2.0, 2.0, 2.0};
    if (argc > 2) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) { printf("cannot open %s\n", argv[2]); return 2; }
        int64_t nv = 0, ne = 0;
        bool ok = fread(&nv, 8, 1, f) == 1 && fread(&ne, 8, 1, f) == 1;
        V.resize((size_t)nv); T.resize((size_t)ne);
        ok = ok && fread(V.data(), sizeof(V[0]), (size_t)nv, f) == (size_t)nv && fread(T.data(), sizeof(T[0]), (size_t)ne, f) == (size_t)ne;
        fclose(f);
        if (!ok) { printf("truncated mesh file\n"); return 2; }
    }
    if (argc > 3) {
        FILE *f = fopen(argv[3], "rb");
        if (!f) { printf("cannot open %s\n", argv[3]); return 2; }
        fseek(f, 0, SEEK_END);
        const long bytes = ftell(f);
        fseek(f, 0, SEEK_SET);
        P.resize((size_t)bytes / sizeof(Real));
        const bool ok = fread(P.data(), sizeof(Real), P.size(), f) == P.size();
        fclose(f);
        if (!ok || P.size() % 3) { printf("bad point file\n"); return 2; }
    }
    try {
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        const size_t nP = P.size() / 3, nNode = sim.numNodes();
        std::vector<Real> field(2 * nNode);
        for (size_t n = 0; n < nNode; ++n) { field[2 * n] = 0.5 * (Real)(n % 11); field[2 * n + 1] = -1.0 + 0.25 * (Real)(n % 5); }
        if (argc > 4) {
            FILE *f = fopen(argv[4], "rb");
            if (!f || fread(field.data(), sizeof(Real), field.size(), f) != field.size()) { printf("cannot read %s\n", argv[4]); return 2; }
            fclose(f);
        }
        const FieldSampler fs(sim);
        std::vector<int32_t> I, I2, NI;
        std::vector<Real> B, C, sqDist, nodeSq;
        fs.closestElementAndBaryCoords(P, I, B);
        fs.closestElementAndPoint(P, sqDist, I2, C);
        fs.closestNodeAndSqDist(P, NI, nodeSq);
        const std::vector<bool> in = fs.contains(P);
        const std::vector<Real> s = fs.sample(P, field, nNode);
        if (I.size() != nP || B.size() != 4 * nP || C.size() != 3 * nP || sqDist.size() != nP || NI.size() != nP || in.size() != nP || s.size() != 2 * nP || I2 != I) {
            printf("FAILED: sizes\n");
            return 2;
        }
        // the raw-mesh sampler: a degree-1 context of its own
        std::vector<Real> vFlat(3 * V.size()), vField(V.size());
        std::vector<int32_t> fFlat(4 * T.size());
        for (size_t v = 0; v < V.size(); ++v) { for (size_t a = 0; a < 3; ++a) vFlat[3 * v + a] = V[v][a]; vField[v] = V[v][0] + 2.0 * V[v][1] - V[v][2]; }
        for (size_t e = 0; e < T.size(); ++e) for (size_t q = 0; q < 4; ++q) fFlat[4 * e + q] = T[e][q];
        const FieldSampler raw(3, vFlat, fFlat, device);
        std::vector<int32_t> rawI;
        std::vector<Real> rawC;
        raw.closestElementAndPoint(P, rawI, rawC);
        const std::vector<Real> rawS = raw.sample(P, vField, V.size());
        bool threw = false;
        try { raw.closestNodeAndSqDist(P, NI, nodeSq); } catch (const std::runtime_error &e) { threw = std::string(e.what()) == "Unsupported for raw meshes"; }
        if (!threw) { printf("FAILED: closestNodeAndSqDist on a raw mesh did not throw\n"); return 2; }
        threw = false;
        try { fs.sample(P, std::vector<Real>(nNode + 1), nNode + 1); } catch (const std::runtime_error &) { threw = true; }
        if (!threw) { printf("FAILED: a field of the wrong length was accepted\n"); return 2; }
        if (rawC != C) { printf("FAILED: the raw-mesh sampler found other closest points\n"); return 2; }
        if (argc > 5) {
            FILE *f = fopen(argv[5], "wb");
            if (!f) { printf("cannot write %s\n", argv[5]); return 2; }
            std::vector<Real> inReal(nP);
            for (size_t i = 0; i < nP; ++i) inReal[i] = in[i] ? 1.0 : 0.0;
            put(f, asReal(I)); put(f, B); put(f, C); put(f, sqDist); put(f, asReal(NI)); put(f, nodeSq); put(f, inReal); put(f, s); put(f, asReal(rawI)); put(f, rawS);
            fclose(f);
        }
        printf("point 0: element %d, squared distance %.17g\n", (int)I[0], sqDist[0]);
        printf("field sampler ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
