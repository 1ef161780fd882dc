// Forms through adjusted points of the bundled block (include/jaicov_forms.h): reads the AICON flat files
// <base>.obc/.scale/.ior/.eor/.phc as example_flatfiles does, adjusts with MatrixInversion::FULL and fits, on the device and with the
// members' whole block of the cofactor matrix, a plane to the first 20 object points of the file and a sphere to the next 8.  The
// points do not lie on forms: the listing shows what the call returns -- parameters, sigma, the global test and the member with the
// largest test -- and agrees with the Python route.
// No Python, no oracle: C++ host mirror + libjaicov_neq.so only.
//   usage: example_forms <base path>
#include <cstdio>
#include <stdexcept>

#include "aicon_reader.hpp"

using namespace jaicov::host;

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <base path of the .obc/.scale/.ior/.eor/.phc files>\n", argv[0]);
        return 2;
    }
    try {
        std::unique_ptr<AiconProject> pr = read_aicon_flat(argv[1]);
        Camera &cam = *pr->camera;
        cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION)->get(3)->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCx()->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCy()->setColumn(COLUMN_FIXED);
        for (auto &p : pr->points)
            if (p->getName().size() > 3) p->setDatum(false);
        BundleAdjustment ba;
        ba.add(&cam);
        for (auto &s : pr->scaleBars) ba.add(s.get());
        ba.setInvertNormalEquation(MatrixInversion::FULL);
        const EstimationStateType state = ba.estimateModel();
        if (state != EstimationStateType::ERROR_FREE_ESTIMATION) {
            std::fprintf(stderr, "error: %s\n", ba.lastError().c_str());
            return 1;
        }
        const double s2 = ba.getVarianceFactorAposteriori();
        std::printf("sigma2 a-posteriori %.17g\n", s2);
        if (pr->points.size() < 28) throw std::runtime_error("fewer than 28 object points in the file");
        const std::vector<int32_t> type = {JAICOV_FORM_PLANE, JAICOV_FORM_SPHERE}, begin = {0, 20, 28};
        std::vector<int32_t> point;
        for (size_t i = 0; i < 28; i++) point.push_back(pr->points[i]->index);
        const BundleAdjustment::FormFits f = ba.fitForms(s2, type, begin, point);
        static const char *name[2] = {"plane", "sphere"};
        for (int g = 0; g < 2; g++) {
            const double *o = &f.table[(size_t)JAICOV_FORM_COLUMNS * g];
            std::printf("form %s status %d iterations %d members", name[g], f.status[g], (int)o[19]);
            for (int i = begin[g]; i < begin[g + 1]; i++) std::printf(" %d", point[i]);
            std::printf("\n  parameters %.17g %.17g %.17g %.17g\n  sigma %.17g %.17g %.17g %.17g\n", o[0], o[1], o[2], o[3], o[7], o[8], o[9], o[10]);
            std::printf("  Omega %.17g f %.17g T %.17g largest distance %.17g rms %.17g\n", o[14], o[15], o[16], o[17], o[18]);
            int worst = begin[g];
            double best = -1.0;                                  // a member without a test (NaN) is never the largest
            for (int i = begin[g]; i < begin[g + 1]; i++)
                if (f.members[(size_t)JAICOV_FORM_MEMBER_COLUMNS * i + 6] > best) { best = f.members[(size_t)JAICOV_FORM_MEMBER_COLUMNS * i + 6]; worst = i; }
            const double *mo = &f.members[(size_t)JAICOV_FORM_MEMBER_COLUMNS * worst];
            std::printf("  largest member test: point %s (index %d) T_i %.17g distance %.17g nabla %.17g\n", pr->points[worst]->getName().c_str(),
                        point[worst], mo[6], mo[3], mo[4]);
        }
        return 0;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
