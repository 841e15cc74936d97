// C++ drop-in test of modalTransient (include/MeshFEMHip/Dynamics.hh) on a quadratic tet Simulator clamped on its face x = min and pulled on its face
// x = max: eight modes computed on the device, static correction, Rayleigh damping, run as two chained halves (the second on the basis the first left
// on the device, started from the first's q, qdot); writes what the two return together; tests/test_cpp_modal_transient.py compares it with one call
// of the Python layer on the same mesh.
// argv: device ordinal, mesh file (i64 nVert, i64 nElem, f64 V[nVert][3], i32 T[nElem][4]), nSteps, density, dt, output file (f64 q[8], qdot[8],
// probes[nSteps + 1][2], modal coordinates[nSteps + 1][8], energies[nSteps + 1][3], the snapshots of every fourth step).
#include <MeshFEMHip/Dynamics.hh>
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
    const int nSteps = argc > 3 ? atoi(argv[3]) : 8;
    const Real density = argc > 4 ? atof(argv[4]) : 1.0;
    const Real dt = argc > 5 ? atof(argv[5]) : 0.1;
    try {
        using Sim = LinearElasticity::Simulator<3, 2>;
        Sim sim(T, V, device);
        sim.setIsotropicMaterial(1.0, 0.3);
        check(sim.ctx(), mfh_set_option(sim.ctx(), "deterministic", 1.0));       // bit-reproducible: the test compares with another process
        sim.applyDirichletBox({-1e-9, -1e-9, -1e-9}, {1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0, 0, 0}, true);
        sim.applyNeumannBox({1.0 - 1e-9, -1e-9, -1e-9}, {1.0 + 1e-9, 1.0 + 1e-9, 1.0 + 1e-9}, {0.0, 0.0, -1.0}, MFH_NEUMANN_TRACTION, true);
        ModalTransientOptions<Sim::VField> opt;
        opt.density = density;
        opt.nModes = 8;
        opt.rayleighMass = 0.05; opt.rayleighStiff = 0.01;
        opt.rtol = 1e-10;
        opt.probes = {{sim.numDoFs() - 1, 2}, {sim.numDoFs() / 2, 0}};
        opt.snapshotStride = 4;
        opt.modalCoords = true;
        opt.energies = true;
        opt.chunkSteps = 32;
        std::vector<Real> amp;
        for (int k = 0; k <= nSteps; ++k) amp.push_back(k % 3 == 0 ? 1.0 : 0.5);
        const int half = nSteps / 2;
        opt.amplitude.assign(amp.begin(), amp.begin() + half + 1);
        const auto r1 = modalTransient(sim, dt, half, opt);
        opt.amplitude.assign(amp.begin() + half, amp.end());
        opt.keepBasis = true;
        opt.q0 = r1.q; opt.qdot0 = r1.qdot;
        auto r = modalTransient(sim, dt, nSteps - half, opt);
        if (r1.info.stepsDone != half || r.info.stepsDone != nSteps - half || half % 4 != 0 || r.q.size() != 8 || r.probes.empty() || r.snapshots.empty() ||
            r1.info.staticSolves != 1) {
            printf("FAILED: steps of the halves\n");
            return 2;
        }
        r.probes.insert(r.probes.begin(), r1.probes.begin(), r1.probes.end() - 1);
        r.modalCoords.insert(r.modalCoords.begin(), r1.modalCoords.begin(), r1.modalCoords.end() - 1);
        r.energies.insert(r.energies.begin(), r1.energies.begin(), r1.energies.end() - 1);
        r.snapshots.insert(r.snapshots.begin(), r1.snapshots.begin(), r1.snapshots.end() - 1);
        if (r.probes.size() != (size_t)nSteps + 1 || r.modalCoords.size() != (size_t)nSteps + 1 || r.snapshots.size() != (size_t)nSteps / 4 + 1 ||
            r.energies.size() != (size_t)nSteps + 1 || r.snapshots[0].size() != sim.numDoFs()) {
            printf("FAILED: sizes\n");
            return 2;
        }
        // a modal and a nodal start together are refused
        bool refused = false;
        opt.u0 = r.snapshots[0];
        try { (void)modalTransient(sim, dt, 2, opt); } catch (const std::runtime_error &) { refused = true; }
        if (!refused) { printf("FAILED: q0 and u0 together were accepted\n"); return 2; }
        if (argc > 6) {
            FILE *f = fopen(argv[6], "wb");
            if (!f) { printf("cannot write %s\n", argv[6]); return 2; }
            fwrite(r.q.data(), sizeof(Real), r.q.size(), f);
            fwrite(r.qdot.data(), sizeof(Real), r.qdot.size(), f);
            for (const auto &p : r.probes) fwrite(p.data(), sizeof(Real), p.size(), f);
            for (const auto &q : r.modalCoords) fwrite(q.data(), sizeof(Real), q.size(), f);
            for (const auto &e : r.energies) fwrite(e.data(), sizeof(Real), 3, f);
            for (const auto &s : r.snapshots) fwrite(&s[0][0], sizeof(Real), 3 * s.size(), f);
            fclose(f);
        }
        printf("%d + %d steps in chunks of %d, %d static iterations\n", half, (int)r.info.stepsDone, (int)r.info.chunkSteps, (int)r1.info.staticIterations);
        printf("modal transient ok\n");
    } catch (const std::runtime_error &e) {
        printf("runtime_error: %s\n", e.what());
        return 3;
    }
    return 0;
}
