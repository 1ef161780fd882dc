// Image space of the bundled block (include/jaicov_predict.h): reads the AICON flat files <base>.obc/.scale/.ior/.eor/.phc as
// example_flatfiles does and adjusts with MatrixInversion::FULL.  Every adjusted object point is then predicted, on the device, into
// every image that does not observe it: the listing counts the predictions that fall into the sensor format (the flat files do not
// carry the sensor size: the format is the box that the block's own measurements span) and shows the largest confidence ellipse
// among them -- the search window a further measurement would need.  The block's own observations are then checked as if they had
// been withheld: every pair comes back with JAICOV_PRED_OBSERVED, which says that Q_ll + J Qxx J' is not their matrix.
// No Python, no oracle: C++ host mirror + libjaicov_neq.so only.
//   usage: example_check_points <base path>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <set>
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
        const auto &f = ba.flat;
        const int nImages = (int)(f.eo_col.size() / 6), nPoints = (int)(f.point_col.size() / 3);
        std::printf("sigma2 a-posteriori %.17g, %d images, %d points, %zu image points\n", s2, nImages, nPoints, f.ip_image.size());
        std::set<std::pair<int, int>> observed;
        double halfW = 0.0, halfH = 0.0;
        for (size_t k = 0; k < f.ip_image.size(); k++) {
            observed.insert({f.ip_image[k], f.ip_point[k]});
            halfW = std::max(halfW, std::fabs(f.ip_x[k]));
            halfH = std::max(halfH, std::fabs(f.ip_y[k]));
        }
        std::vector<int32_t> images, points;
        for (int i = 0; i < nImages; i++)
            for (int p = 0; p < nPoints; p++)
                if (!observed.count({i, p})) { images.push_back(i); points.push_back(p); }
        const double k2 = 2.4477;                       // sqrt of the 95 % quantile of chi^2 with 2 degrees of freedom
        const BundleAdjustment::ImageTable t = ba.predictImagePoints(s2, images, points, k2);
        size_t inside = 0, flagged = 0, largest = images.size();
        for (size_t k = 0; k < images.size(); k++) {
            const double *o = &t.table[(size_t)JAICOV_PRED_POINT_COLUMNS * k];
            if (t.status[k] & (JAICOV_PRED_NOT_FINITE | JAICOV_PRED_OBSERVED)) { flagged++; continue; }
            if (!(std::fabs(o[0]) <= halfW && std::fabs(o[1]) <= halfH)) continue;
            inside++;
            if (largest == images.size() || o[7] > t.table[(size_t)JAICOV_PRED_POINT_COLUMNS * largest + 7]) largest = k;
        }
        std::printf("unobserved pairs %zu, predicted inside the format +-%.3f x +-%.3f mm: %zu (not finite or observed: %zu)\n", images.size(), halfW,
                    halfH, inside, flagged);
        if (largest < images.size()) {
            const double *o = &t.table[(size_t)JAICOV_PRED_POINT_COLUMNS * largest];
            std::printf("largest 95 %% ellipse: point %s in image %d at (%.4f, %.4f) mm, sigma (%.5f, %.5f) mm, semi-axes %.5f x %.5f mm, direction %.4f rad\n",
                        ba.getObjectCoordinates()[points[largest]]->getName().c_str(), images[largest], o[0], o[1], o[5], o[6], o[7], o[8], o[9]);
        }
        // the block's own observations as if withheld
        std::vector<double> xy, disp;
        for (size_t k = 0; k < f.ip_image.size(); k++) {
            xy.push_back(f.ip_x[k]); xy.push_back(f.ip_y[k]);
            disp.push_back(f.ip_var_x[k]); disp.push_back(f.ip_var_y[k]); disp.push_back(f.ip_rho[k]);
        }
        const BundleAdjustment::ImageCheck c = ba.checkImagePoints(f.ip_image, f.ip_point, xy, disp, s2);
        size_t flaggedObserved = 0;
        double worstT = 0.0;
        for (size_t k = 0; k < c.status.size(); k++) {
            if (c.status[k] & JAICOV_PRED_OBSERVED) flaggedObserved++;
            worstT = std::max(worstT, c.table[(size_t)JAICOV_PRED_CHECK_COLUMNS * k + 7]);
        }
        std::printf("own observations re-checked: %zu of %zu flagged OBSERVED (their matrix is Q_ll - J Qxx J', not the sum), largest T_post %.4f\n",
                    flaggedObserved, c.status.size(), worstT);
        return flaggedObserved == c.status.size() ? 0 : 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
