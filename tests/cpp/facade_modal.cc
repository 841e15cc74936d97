// C++ drop-in test of modalFrequencyResponse (include/MeshFEMHip/Harmonic.hh) on a quadratic tet Simulator clamped on its face x = min and pulled on
// its face x = max: eight modes computed on the device, static correction, a true residual at every second frequency; writes what it returns for three
// frequencies; tests/test_cpp_modal.py compares it with the Python layer's on the same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), density, three frequencies, output file (per frequency the
// field as {re, im} pairs [nDoF][3][2], then the probes [3][2][2], the modal coordinates [3][8][2], the true residuals [3] and the eigenvalues [8]).
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
    std::vector<Real> omegas = {0.0, 0.1, 0.2};
    for (int k = 0; k < 3; ++k)
        if (argc > 4 + k) omegas[(size_t)k] = atof(argv[4 + k]);
    try {
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0, 0, 0}, true);
        sim.applyNeumannBox({1.0 - 1e-9, -1e-9, -1e-9}, {1.0 + 1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0.0, 0.0, -1.0}, MFH_NEUMANN_TRACTION, true);
        ModalHarmonicOptions<Sim::VField> opt;
        opt.density = density;
        opt.nModes = 8;
        opt.rayleighMass = 0.05; opt.rayleighStiff = 0.01; opt.lossFactor = 0.02;
        opt.rtol = 1e-10;
        opt.residualStride = 2;
        opt.probes = {{sim.numDoFs() - 1, 2}, {sim.numDoFs() / 2, 0}};
        const auto r = modalFrequencyResponse(sim, omegas, opt);
        if (r.basisInfo.nModes != 8 || r.u.size() != 3 || r.u[0].size() != sim.numDoFs() || r.probes.size() != 3 || r.probes[0].size() != 2 ||
            r.modalCoords.size() != 3 || r.modalCoords[0].size() != 8 || r.trueResiduals.size() != 3 || r.lambda.size() != 8) {
            printf("FAILED: sizes\n");
            return 2;
        }
        if (argc > 7) {
            FILE *f = fopen(argv[7], "wb");
            if (!f) { printf("cannot write %s\n", argv[7]); return 2; }
            for (const auto &u : r.u) fwrite(&u[0][0], sizeof(std::complex<Real>), 3 * u.size(), f);
            for (const auto &p : r.probes) fwrite(p.data(), sizeof(std::complex<Real>), p.size(), f);
            for (const auto &q : r.modalCoords) fwrite(q.data(), sizeof(std::complex<Real>), q.size(), f);
            fwrite(r.trueResiduals.data(), sizeof(Real), r.trueResiduals.size(), f);
            fwrite(r.lambda.data(), sizeof(Real), r.lambda.size(), f);
            fclose(f);
        }
        printf("%d modes (defect %.2e), %d static solves (%d iterations), %d group(s) of %d planes per pass, worst true residual %.2e, note: %s\n",
               (int)r.basisInfo.nModes, r.basisInfo.orthoDefect, (int)r.info.staticSolves, (int)r.info.staticIterations, (int)r.info.groups,
               (int)r.info.planesPerPass, r.info.worstTrueResidual, r.info.note);
        printf("modal ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
