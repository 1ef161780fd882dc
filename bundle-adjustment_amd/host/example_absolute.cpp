// The bundled block adjusted from a model that is grown from its image measurements and the .ior camera alone and then carried onto the
// .obc coordinates by an absolute orientation: reads the AICON flat files <base>.obc/.scale/.ior/.eor/.phc as example_flatfiles does,
// keeps the .obc coordinates as the target frame and ignores the .eor orientations.
//   1-3. the model of all images and points, in the frame of the pair's first image with base length 1 (model_growth.hpp, the steps
//        of example_relative);
//   4. the similarity transformation of the model onto the .obc coordinates over all common points (SimilarityTransformation::
//      estimateAll = jaicov_simil_models): once with unit weights, which gives the standard deviation of a coordinate, then with that
//      variance as the target's cofactors and rejection at 5 sigma; SimilarityTransformation::apply (= jaicov_simil_apply) carries every
//      point and every exterior orientation into the .obc frame;
//   5. estimateModel() runs with MatrixInversion::REDUCED.
// No scale bar is needed for the start values: the scale comes out of the transformation.
//   usage: example_absolute <base path>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "model_growth.hpp"

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
        // the target frame: the .obc coordinates, kept before the model forgets them
        SimilarityTransformation::Model model;
        for (auto &p : pr->points) {
            model.points.push_back(p.get());
            model.target.push_back({p->getX().getValue(), p->getY().getValue(), p->getZ().getValue()});
        }
        growth::grow_model(*pr, cam);                                         // steps 1 to 3, reported line by line

        // 4. the model onto the .obc coordinates
        const int n = (int)model.points.size();
        SimilarityTransformation::Result r = SimilarityTransformation::estimateAll({model})[0];
        if (r.status != JAICOV_SIMIL_OK) throw std::runtime_error("the similarity transformation failed with status " + std::to_string(r.status));
        const double s2 = r.values[35] / (3.0 * n - 7.0);
        std::printf("unit weights                  %d points, %d Gauss-Newton steps, sigma of a coordinate %.6f\n", n, r.iterations, std::sqrt(s2));
        if (s2 > 0.0) {
            model.cofTarget.assign(n, std::array<double, 6>{s2, 0.0, 0.0, s2, 0.0, s2});
            r = SimilarityTransformation::estimateAll({model}, 5.0, 4)[0];
            if (r.status != JAICOV_SIMIL_OK) throw std::runtime_error("the similarity transformation failed with status " + std::to_string(r.status));
        }
        const int dof = 3 * r.pointsUsed - 7;
        const double s02 = dof > 0 ? r.values[35] / dof : 0.0;   // the variance factor over the second run's cofactors, which are variances
        std::printf("similarity transformation     status %d, start kind %d, %d Gauss-Newton steps, %d of %d points used\n", r.status, r.startKind,
                    r.iterations, r.pointsUsed, r.points);
        static const char *const names[7] = {"translation X", "translation Y", "translation Z", "scale m", "omega", "phi", "kappa"};
        for (int k = 0, d = 7; k < 7; d += 7 - k, k++)            // d: the diagonal entry of row k in the packed upper triangle
            std::printf("%-29s %.9f +- %.3e\n", names[k], r.values[k], std::sqrt(s02 * r.values[d]));
        std::printf("Omega / sigma0                %.6e / %.6f\n", r.values[35], std::sqrt(s02));
        for (int k = 0; k < n; k++)
            if (!r.used[k]) std::printf("withdrawn                     point %s, q %.3f\n", model.points[k]->getName().c_str(), r.q[k]);
        std::vector<Image *> images;
        for (auto &im : cam.images()) images.push_back(im.get());
        if (!SimilarityTransformation::apply(r, model.points, images)) throw std::runtime_error("the model could not be carried over");
        double worst = 0.0;
        for (int k = 0; k < n; k++) {
            const double d[3] = {model.points[k]->getX().getValue() - model.target[k][0], model.points[k]->getY().getValue() - model.target[k][1],
                                 model.points[k]->getZ().getValue() - model.target[k][2]};
            if (r.used[k]) worst = std::max(worst, std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
        }
        std::printf("largest distance to .obc      %.6f (used points)\n", worst);
        std::printf("start values                  %.3f sec\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());

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
