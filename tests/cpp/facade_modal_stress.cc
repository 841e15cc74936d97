// C++ drop-in test of modalRandomStress and responseSpectrumStress (include/MeshFEMHip/Harmonic.hh) on a quadratic tet Simulator clamped on its face
// x = min and pulled on its face x = max: eight modes computed on the device, 3 % modal damping, the static correction, RMS von Mises and
// components; then the CQC peak stress of a base motion in z. tests/test_cpp_modal_stress.py compares what it writes with the Python layer's on the
// same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), density, output file (von Mises [nElem][4], components
// [nElem][4][6], peak value, peak element, peak corner, C^(0) [nb][nb], lambda [8]; von Mises [nElem][4] of the response spectrum, its peak value,
// element and corner, gamma [8]).
#include <MeshFEMHip/Harmonic.hh>
#include <cstdio>
#include <cstdlib>

using namespace MeshFEMHip;

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
    const Real density = argc > 3 ? atof(argv[3]) : 1.0;
    const size_t nFreq = 40;
    std::vector<Real> omegas(nFreq);
    std::vector<std::complex<Real>> S(nFreq);
    for (size_t k = 0; k < nFreq; ++k) {
        omegas[k] = 0.02 + 0.015 * (Real)k;
        S[k] = 1.0 / (1.0 + omegas[k] * omegas[k]);
    }
    try {
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0, 0, 0}, true);
        sim.applyNeumannBox({1.0 - 1e-9, -1e-9, -1e-9}, {1.0 + 1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0.0, 0.0, -1.0}, MFH_NEUMANN_TRACTION, true);
        ModalRandomOptions<Sim::VField> opt;
        opt.density = density;
        opt.nModes = 8;
        opt.modalDamping.assign(8, 0.03);
        opt.rtol = 1e-10;
        ModalStressOptions sopt;
        sopt.components = true;
        const auto r = modalRandomStress(sim, omegas, S, opt, sopt);
        const size_t corners = sim.numElements() * 4;
        if (r.basisInfo.nModes != 8 || r.vonMises.size() != corners || r.components.size() != corners * 6 || r.info.nb != 9 || r.cov.size() != 81 ||
            r.lambda.size() != 8 || r.peakElement >= sim.numElements() || r.peakCorner >= 4 || r.vonMises[r.peakElement * 4 + r.peakCorner] != r.peakVonMises) {
            printf("FAILED: sizes or peak\n");
            return 2;
        }
        ResponseSpectrumOptions<Sim::VField> so;
        so.density = density;
        so.nModes = 8;
        so.zeta = 0.05;
        const auto q = responseSpectrumStress(sim, 2, [](Real w, Real z) { return 0.3 / (w * w) * (1.0 + z); }, so);
        if (q.vonMises.size() != corners || !q.components.empty() || q.gamma.size() != 8 || q.info.ranks[0] < 1) {
            printf("FAILED: sizes of the response spectrum\n");
            return 2;
        }
        if (argc > 4) {
            FILE *f = fopen(argv[4], "wb");
            if (!f) { printf("cannot write %s\n", argv[4]); return 2; }
            const Real peak[3] = {r.peakVonMises, (Real)r.peakElement, (Real)r.peakCorner}, qpeak[3] = {q.peakVonMises, (Real)q.peakElement, (Real)q.peakCorner};
            fwrite(r.vonMises.data(), sizeof(Real), r.vonMises.size(), f);
            fwrite(r.components.data(), sizeof(Real), r.components.size(), f);
            fwrite(peak, sizeof(Real), 3, f);
            fwrite(r.cov.data(), sizeof(Real), r.cov.size(), f);
            fwrite(r.lambda.data(), sizeof(Real), r.lambda.size(), f);
            fwrite(q.vonMises.data(), sizeof(Real), q.vonMises.size(), f);
            fwrite(qpeak, sizeof(Real), 3, f);
            fwrite(q.gamma.data(), sizeof(Real), q.gamma.size(), f);
            fclose(f);
        }
        printf("%d modes, %d static solve(s), rank %d in %d pass(es), truncation %.2e, peak von Mises %.4e at element %d corner %d; response spectrum: rank %d, note: %s\n",
               (int)r.basisInfo.nModes, (int)r.info.staticSolves, (int)r.info.ranks[0], (int)r.info.passes[0], r.info.truncation[0], r.peakVonMises,
               (int)r.peakElement, (int)r.peakCorner, (int)q.info.ranks[0], r.info.note);
        printf("modal stress ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
