// The bundled block's start values built from image coordinates that are corrected for lens distortion, beside the same start values
// built from the measured ones: reads the AICON flat files <base>.obc/.scale/.ior/.eor/.phc as example_absolute does, keeps the .obc
// coordinates as the target frame and ignores the .eor orientations.  Twice, first with and then without the correction:
//   0. (with the correction) LensCorrection::correctAll (= jaicov_lens_correct) reduces every image coordinate to the distortion-free
//      camera of the .ior file, and a LensCorrection::Scope holds the corrected values and dispersions in the ImageCoordinates;
//   1-3. the model of all images and points is grown (model_growth.hpp, the steps of example_relative and example_absolute);
//   4. the similarity transformation over all common points, as in example_absolute, carries it onto the .obc coordinates;
//   the Scope ends here, and the measured coordinates are back;
//   5. estimateModel() runs with MatrixInversion::REDUCED on the measured coordinates: the adjustment models the distortion itself.
// The relative orientation's Omega and steps (reported by step 1), the number of adjustment passes and sigma0 of both runs end the output.
//   usage: example_corrected_start <base path>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "model_growth.hpp"

using namespace jaicov::host;

namespace {

struct Outcome {
    int passes = 0;
    double sigma0 = 0.0, seconds = 0.0;
    bool ok = false;
};

// 4. the model onto the .obc coordinates: unit weights, then the coordinate variance they give as the target's cofactors and rejection
void carry_onto_target(SimilarityTransformation::Model &model, Camera &cam) {
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
    std::printf("similarity transformation     status %d, %d Gauss-Newton steps, %d of %d points used, scale m %.9f\n", r.status, r.iterations,
                r.pointsUsed, r.points, r.values[3]);
    std::vector<Image *> images;
    for (auto &im : cam.images()) images.push_back(im.get());
    if (!SimilarityTransformation::apply(r, model.points, images)) throw std::runtime_error("the model could not be carried over");
}

Outcome run(const char *base, bool corrected) {
    const auto t0 = std::chrono::steady_clock::now();
    std::printf("start values from %s coordinates\n", corrected ? "corrected" : "measured");
    std::unique_ptr<AiconProject> pr = read_aicon_flat(base);
    Camera &cam = *pr->camera;
    cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION)->get(3)->setColumn(COLUMN_FIXED);
    cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCx()->setColumn(COLUMN_FIXED);
    cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCy()->setColumn(COLUMN_FIXED);
    for (auto &p : pr->points)
        if (p->getName().size() > 3) p->setDatum(false);
    SimilarityTransformation::Model model;
    for (auto &p : pr->points) {
        model.points.push_back(p.get());
        model.target.push_back({p->getX().getValue(), p->getY().getValue(), p->getZ().getValue()});
    }
    {
        std::unique_ptr<LensCorrection::Scope> scope;
        if (corrected) {
            const std::vector<LensCorrection::Result> res = LensCorrection::correctAll(cam);
            int solves = 0, failed = 0;
            double shift = 0.0;
            for (const LensCorrection::Result &r : res) {
                if (r.status != JAICOV_LENS_OK) { failed++; continue; }
                solves = std::max(solves, r.iterations);
                shift = std::max(shift, std::max(std::fabs(r.x - r.coordinate->getX().getValue()), std::fabs(r.y - r.coordinate->getY().getValue())));
            }
            std::printf("lens correction               %zu image points, %d without a result, at most %d solves, largest shift %.6f\n", res.size(),
                        failed, solves, shift);
            scope.reset(new LensCorrection::Scope(res));
        }
        growth::grow_model(*pr, cam);                                     // steps 1 to 3, reported line by line
        carry_onto_target(model, cam);
    }                                                                     // the measured coordinates are back
    BundleAdjustment ba;
    ba.add(&cam);
    for (auto &s : pr->scaleBars) ba.add(s.get());
    ba.setInvertNormalEquation(MatrixInversion::REDUCED);
    const EstimationStateType state = ba.estimateModel();
    Outcome o;
    o.ok = state == EstimationStateType::ERROR_FREE_ESTIMATION;
    o.passes = ba.getIterations();
    o.sigma0 = std::sqrt(ba.getVarianceFactorAposteriori());
    o.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("state                         %d%s\n", (int)state, o.ok ? " (ERROR_FREE_ESTIMATION)" : "");
    if (!ba.lastError().empty()) std::printf("engine                        %s\n", ba.lastError().c_str());
    std::printf("iterations                    %d\n", o.passes);
    std::printf("sigma0 a-posteriori           %.9f\n", o.sigma0);
    std::printf("time                          %.3f sec\n\n", o.seconds);
    return o;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <base path of the .obc/.scale/.ior/.eor/.phc files>\n", argv[0]);
        return 2;
    }
    try {
        const Outcome c = run(argv[1], true), m = run(argv[1], false);
        std::printf("adjustment passes             %d from corrected, %d from measured coordinates\n", c.passes, m.passes);
        std::printf("sigma0                        %.9f from corrected, %.9f from measured coordinates\n", c.sigma0, m.sigma0);
        return c.ok && m.ok ? 0 : 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
