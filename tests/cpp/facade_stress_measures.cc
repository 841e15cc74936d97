// C++ drop-in test of include/MeshFEMHip/VonMises.hh and FieldPostProcessing.hh on a quadratic tet Simulator: prints what the free functions
// return; tests/test_cpp_stress_measures.py compares the numbers with the numpy restatement of the reference's routines.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), displacement file (f64 u[nNode][3]), output file.
// Output: f64 stress field [nElem][4][6], von Mises of it, eigenvalues of it, fused von Mises, fused eigenvalues, peak value, peak index (as
// f64), vertex average of the stress field [nVert][6], the one-call vertex-averaged stress, vertex average of a per-element scalar [nVert].
#include <MeshFEMHip/FieldPostProcessing.hh>
#include <MeshFEMHip/VonMises.hh>
#include <cstdio>
#include <cstdlib>

using namespace MeshFEMHip;

static void put(FILE *f, const Real *p, size_t n) { fwrite(p, sizeof(Real), n, f); }

int main(int argc, char **argv) {
    const int device = argc > 1 ? atoi(argv[1]) : 0;
    std::vector<std::array<Real, 3>> V = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};      // one tetrahedron: enough to reach the device (or fail to)
    std::vector<std::array<int32_t, 4>> T = {{0, 1, 2, 3}};
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
    try {
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        Sim::VField u(sim.numNodes());
        for (size_t n = 0; n < u.size(); ++n) u[n] = {0.1 * (Real)n, -0.05 * (Real)(n % 7), 0.02 * (Real)(n % 3)};
        if (argc > 3) {
            FILE *f = fopen(argv[3], "rb");
            if (!f || fread(u.data(), sizeof(u[0]), u.size(), f) != u.size()) { printf("cannot read %s\n", argv[3]); return 2; }
            fclose(f);
        }
        const size_t nElem = sim.numElements(), nCorner = 4 * nElem;
        const std::vector<Real> flat = sim.stressField(u);
        Sim::SMField sigma(nCorner);
        for (size_t k = 0; k < nCorner; ++k)
            for (size_t c = 0; c < 6; ++c) sigma[k][c] = flat[6 * k + c];
        const std::vector<Real> vm = vonMises(sim, sigma), ev = eigenvalues(sim, sigma), vmOwn = vonMises(sigma);
        const auto dec = eigenDecomposition(sim.ctx(), sigma);
        const std::vector<Real> vmFused = vonMisesStress(sim, u), evFused = principalStresses(sim, u);
        const auto peak = peakVonMises(sim, u);
        const Sim::SMField avg = vertexAveragedField(sim, sigma), avgOne = vertexAveragedStress(sim, u);
        std::vector<Real> perElem(nElem);
        for (size_t e = 0; e < nElem; ++e) perElem[e] = 1.0 + 0.25 * (Real)(e % 5);
        const std::vector<Real> avgScalar = vertexAveragedField(sim, perElem);
        if (vm.size() != nCorner || ev.size() != 3 * nCorner || dec.second.size() != 9 * nCorner || vmFused.size() != nCorner || evFused.size() != 3 * nCorner ||
            avg.size() != V.size() || avgOne.size() != V.size() || avgScalar.size() != V.size() || vmOwn != vm || dec.first != ev) {
            printf("FAILED: sizes\n");
            return 2;
        }
        bool threw = false;
        try { vertexAveragedField(sim, std::vector<Real>(nElem + 1)); } catch (const std::runtime_error &) { threw = true; }
        if (!threw) { printf("FAILED: a field of the wrong length was accepted\n"); return 2; }
        if (argc > 4) {
            FILE *f = fopen(argv[4], "wb");
            if (!f) { printf("cannot write %s\n", argv[4]); return 2; }
            const Real pk[2] = {peak.first, (Real)peak.second};
            put(f, flat.data(), flat.size()); put(f, vm.data(), vm.size()); put(f, ev.data(), ev.size());
            put(f, vmFused.data(), vmFused.size()); put(f, evFused.data(), evFused.size()); put(f, pk, 2);
            put(f, &avg[0][0], 6 * avg.size()); put(f, &avgOne[0][0], 6 * avgOne.size()); put(f, avgScalar.data(), avgScalar.size());
            fclose(f);
        }
        printf("peak von Mises %.17g at corner %lld\n", peak.first, (long long)peak.second);
        printf("stress measures ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
