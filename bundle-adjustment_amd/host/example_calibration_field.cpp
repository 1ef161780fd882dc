// The bundled camera in image space (include/jaicov_calibration.h): reads the AICON flat files <base>.obc/.scale/.ior/.eor/.phc as
// example_flatfiles does, adjusts the block with MatrixInversion::REDUCED (the mode of the reference's examples: the cofactor matrix
// holds no column of an exterior orientation, and none is needed) and prints the radial profile dr(r) +- sigma of the camera's
// image correction in steps of 1 mm, the 9 x 7 grid of its sigma ellipses over the sensor, and the comparison of the adjusted camera
// with its own values as a reference set (a zero field).
// No Python, no oracle: C++ host mirror + libjaicov_neq.so only.
//   usage: example_calibration_field <base path>
#include <cmath>
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
        const std::string base = argv[1];
        std::unique_ptr<AiconProject> owner(new AiconProject());
        AiconProject &pr = *owner;
        read_obc(pr, base + ".obc");
        read_ior(pr, base + ".ior");
        read_scale(pr, base + ".scale");
        read_eor(pr, base + ".eor");
        for_each_line(base + ".phc", [&](const std::string &line) {                     // PHCFileReader.java:74-117
            auto col = split_ws(line);
            if (col.size() < 11 || !(std::stoi(col[9]) > 0)) return;
            Image *im = pr.camera->add(std::stol(col[0]));
            auto it = pr.byName.find(col[1]);
            if (it == pr.byName.end()) return;
            im->add(it->second, std::stod(col[2]), std::stod(col[3]), std::stod(col[4]), std::stod(col[5]));
        });
        // the sensor format is the fifth line of the .ior file (width, height in mm)
        double width = 36.0, height = 24.0;
        int lineNo = 0;
        for_each_line(base + ".ior", [&](const std::string &line) {
            auto col = split_ws(line);
            if (col.empty()) return;
            if (++lineNo == 5 && col.size() >= 2) { width = std::stod(col[0]); height = std::stod(col[1]); }
        });
        Camera &cam = *pr.camera;
        cam.getDistortionModel(DistortionModel::Type::RADIAL_DISTORTION)->get(3)->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCx()->setColumn(COLUMN_FIXED);
        cam.getDistortionModel(DistortionModel::Type::AFFINITY_AND_SHEAR)->getCy()->setColumn(COLUMN_FIXED);
        for (auto &p : pr.points)
            if (p->getName().size() > 3) p->setDatum(false);
        BundleAdjustment ba;
        ba.add(&cam);
        for (auto &s : pr.scaleBars) ba.add(s.get());
        ba.setInvertNormalEquation(MatrixInversion::REDUCED);
        const EstimationStateType state = ba.estimateModel();
        if (state != EstimationStateType::ERROR_FREE_ESTIMATION) {
            std::fprintf(stderr, "error: %s\n", ba.lastError().c_str());
            return 1;
        }
        const double s2 = ba.getVarianceFactorAposteriori();
        std::printf("sigma2 a-priori %.6g, a-posteriori %.6g, degrees of freedom %d; sensor %.3f x %.3f mm\n", ba.getVarianceFactorApriori(), s2,
                    ba.getDegreeOfFreedom(), width, height);
        // the radial profile along +x
        const int nr = (int)std::floor(0.5 * std::hypot(width, height));
        std::vector<int32_t> cams(nr, 0);
        std::vector<double> xy(2 * nr, 0.0);
        for (int k = 0; k < nr; k++) xy[2 * k] = k + 1.0;
        const BundleAdjustment::CalibrationField prof = ba.calibrationField(s2, cams, xy);
        std::printf("radial profile along +x (mm): r, dr +- sigma, dt +- sigma, status\n");
        bool ok = true;
        for (int k = 0; k < nr; k++) {
            const double *o = &prof.table[(size_t)JAICOV_CALIB_FIELD_COLUMNS * k];
            std::printf("profile %5.1f  %+.6f +- %.6f  %+.6f +- %.6f  %d\n", xy[2 * k], o[10], o[12], o[11], o[13], prof.status[k]);
            ok = ok && std::isfinite(o[10]) && o[12] > 0.0 && !(prof.status[k] & (JAICOV_CALIB_NOT_FINITE | JAICOV_CALIB_NEGATIVE));
        }
        // the 9 x 7 grid of sigma ellipses (expansion factor 1)
        const int nx = 9, ny = 7;
        std::vector<int32_t> gcams(nx * ny, 0);
        std::vector<double> gxy;
        for (int j = 0; j < ny; j++)
            for (int i = 0; i < nx; i++) {
                gxy.push_back(-0.5 * width + width * i / (nx - 1));
                gxy.push_back(-0.5 * height + height * j / (ny - 1));
            }
        const BundleAdjustment::CalibrationField grid = ba.calibrationField(s2, gcams, gxy);
        std::printf("sigma ellipses over the sensor (mm): xs, ys, dx, dy, semi-axes A x B, direction (rad), status\n");
        double largest = 0.0;
        for (int k = 0; k < nx * ny; k++) {
            const double *o = &grid.table[(size_t)JAICOV_CALIB_FIELD_COLUMNS * k];
            std::printf("ellipse %8.3f %8.3f  %+.6f %+.6f  %.6f x %.6f  %.4f  %d\n", gxy[2 * k], gxy[2 * k + 1], o[0], o[1], o[7], o[8], o[9], grid.status[k]);
            ok = ok && o[7] >= o[8] && o[8] >= 0.0 && !(grid.status[k] & (JAICOV_CALIB_NOT_FINITE | JAICOV_CALIB_NEGATIVE));
            largest = std::fmax(largest, o[7]);
        }
        std::printf("largest semi-axis on the grid: %.6f mm\n", largest);
        // the adjusted camera against its own values as a reference set: the difference field is zero to the bit
        const BundleAdjustment::CalibrationCompare self = ba.compareCalibration(0, 0, gxy, {}, ba.cameraValues(0), {}, s2, true);
        std::printf("adjusted camera against itself on the grid: rms %.3g mm, rms expected %.6f mm, max |d| %.3g mm at node %.0f\n", self.summary[1],
                    self.summary[2], self.summary[3], self.summary[4]);
        ok = ok && self.summary[0] == nx * ny && self.summary[1] == 0.0 && self.summary[3] == 0.0 && self.summary[4] == 0.0;
        return ok ? 0 : 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
