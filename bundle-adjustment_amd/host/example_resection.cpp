// The bundled block adjusted from resected start values of its exterior orientations: reads the AICON flat files
// <base>.obc/.scale/.ior/.eor/.phc as example_flatfiles does, computes the orientation of every image from the .obc points it sees and
// the .ior camera (SpatialResection::resectAll, one device call for all images, linear start; the .eor values are ignored), prints the
// largest difference of a resected orientation from its .eor value, then runs estimateModel() with MatrixInversion::REDUCED.
//   usage: example_resection <base path>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "aicon_reader.hpp"

using namespace jaicov::host;

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <base path of the .obc/.scale/.ior/.eor/.phc files>\n", argv[0]);
        return 2;
    }
    const auto t0 = std::chrono::steady_clock::now();
    try {
        std::unique_ptr<AiconProject> pr = read_aicon_flat(argv[1]);
        Camera &cam = *pr->camera;
        cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION)->get(3)->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCx()->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCy()->setColumn(COLUMN_FIXED);
        for (auto &p : pr->points)
            if (p->getName().size() > 3) p->setDatum(false);

        // every image from the object points it sees, one device call
        std::map<Image *, std::array<double, 6>> eor;
        for (auto &im : cam.images())
            for (int k = 0; k < 6; k++) eor[im.get()][k] = im->getExteriorOrientation().at(k)->getValue();
        const auto ti = std::chrono::steady_clock::now();
        const std::vector<SpatialResection::Result> res = SpatialResection::resectAll({&cam});
        const double resect_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - ti).count();
        int count[5] = {0, 0, 0, 0, 0}, kinds[3] = {0, 0, 0}, max_iter = 0;
        double maxd = 0.0, maxa = 0.0;
        for (const SpatialResection::Result &r : res) {
            count[r.status]++;
            if (r.status != JAICOV_RESECT_OK && r.status != JAICOV_RESECT_NOT_CONVERGED) continue;
            kinds[r.startKind]++;
            const std::array<double, 6> &e = eor[r.image];
            for (int k = 0; k < 3; k++) maxd = std::max(maxd, std::fabs(r.values[k] - e[k]));
            for (int k = 3; k < 6; k++) maxa = std::max(maxa, std::fabs(std::remainder(r.values[k] - e[k], 2.0 * M_PI)));
            max_iter = std::max(max_iter, r.iterations);
        }
        std::printf("resected images               %zu (%.3f sec)\n", res.size(), resect_secs);
        std::printf("status ok / not converged     %d / %d\n", count[0], count[1]);
        std::printf("too few points / singular / nan %d / %d / %d (these keep their .eor orientation)\n", count[2], count[3], count[4]);
        std::printf("space / plane starts          %d / %d\n", kinds[1], kinds[2]);
        std::printf("most Gauss-Newton steps       %d\n", max_iter);
        std::printf("max |resected - eor|          %.6f mm, %.9f rad\n", maxd, maxa);

        BundleAdjustment ba;
        ba.add(&cam);
        for (auto &s : pr->scaleBars) ba.add(s.get());
        ba.setInvertNormalEquation(MatrixInversion::REDUCED);
        ba.addPropertyChangeListener([](const std::string &name, double a, double b) {
            if (name == "CONVERGENCE") std::printf("  max|dx| = %.3e (threshold %.3e)\n", b, a);
        });
        const EstimationStateType state = ba.estimateModel();
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("state                      %d%s\n", (int)state, state == EstimationStateType::ERROR_FREE_ESTIMATION ? " (ERROR_FREE_ESTIMATION)" : "");
        if (!ba.lastError().empty()) std::printf("engine                     %s\n", ba.lastError().c_str());
        std::printf("iterations                 %d\n", ba.getIterations());
        std::printf("omega                      %.10e\n", ba.getOmega());
        std::printf("sigma0 a-posteriori        %.9f\n", std::sqrt(ba.getVarianceFactorAposteriori()));
        std::printf("Estimation time: %.3f sec\n", secs);
        return state == EstimationStateType::ERROR_FREE_ESTIMATION ? 0 : 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
