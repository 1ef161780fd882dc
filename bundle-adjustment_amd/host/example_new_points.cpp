// Object space of the bundled block (include/jaicov_newpoints.h): reads the AICON flat files <base>.obc/.scale/.ior/.eor/.phc as
// example_flatfiles does, but withholds the image measurements of every tenth object point (the ends of the scale bars stay), and
// adjusts the rest with MatrixInversion::FULL.  The withheld points are then intersected on the device as new points from their
// withheld measurements (an even selection of 64 where a point has more: the limit of the call), starting from their .obc coordinates.  The listing shows X, Y, Z of every such point with its sigmas from
// the measurement noise alone (Q_meas) and from Q_XX = Q_meas + Q_sys, which carries the uncertainty of the camera and the stations
// out of the full Qxx, and the length between the first two with its cofactor with and without their correlations.
// No Python, no oracle: C++ host mirror + libjaicov_neq.so only.
//   usage: example_new_points <base path>
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
        const std::string base = argv[1];
        std::unique_ptr<AiconProject> owner(new AiconProject());
        AiconProject &pr = *owner;
        read_obc(pr, base + ".obc");
        read_ior(pr, base + ".ior");
        read_scale(pr, base + ".scale");
        read_eor(pr, base + ".eor");
        std::set<ObjectCoordinate *> keep, withheld;
        for (auto &s : pr.scaleBars) { keep.insert(s->getObjectCoordinateA()); keep.insert(s->getObjectCoordinateB()); }
        std::vector<ObjectCoordinate *> fresh;
        for (size_t k = 9; k < pr.points.size(); k += 10)
            if (!keep.count(pr.points[k].get())) { withheld.insert(pr.points[k].get()); fresh.push_back(pr.points[k].get()); }
        // PHCFileReader.java:74-117, the measurements of the withheld points set aside
        struct Ray { Image *image; double x, y, sx, sy; };
        std::vector<std::vector<Ray>> rays(fresh.size());
        for_each_line(base + ".phc", [&](const std::string &line) {
            auto col = split_ws(line);
            if (col.size() < 11 || !(std::stoi(col[9]) > 0)) return;
            Image *im = pr.camera->add(std::stol(col[0]));
            auto it = pr.byName.find(col[1]);
            if (it == pr.byName.end()) return;
            const double xp = std::stod(col[2]), yp = std::stod(col[3]), sx = std::stod(col[4]), sy = std::stod(col[5]);
            if (!withheld.count(it->second)) { im->add(it->second, xp, yp, sx, sy); return; }
            const size_t i = std::find(fresh.begin(), fresh.end(), it->second) - fresh.begin();
            rays[i].push_back({im, xp, yp, sx, sy});
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
        ba.setInvertNormalEquation(MatrixInversion::FULL);
        const EstimationStateType state = ba.estimateModel();
        if (state != EstimationStateType::ERROR_FREE_ESTIMATION) {
            std::fprintf(stderr, "error: %s\n", ba.lastError().c_str());
            return 1;
        }
        const double s2 = ba.getVarianceFactorAposteriori();
        std::printf("sigma2 a-posteriori %.17g, %zu points adjusted, %zu points withheld\n", s2, ba.flat.point_col.size() / 3, fresh.size());
        std::vector<int32_t> rayBegin{0}, rayImage, pairs;
        std::vector<double> xy, disp, start;
        for (size_t i = 0; i < fresh.size(); i++) {
            // a new point takes JAICOV_NEWPT_MAX_RAYS rays at most; the block's points are seen in up to 93 images: an even selection of 64
            const size_t m = rays[i].size(), take = std::min<size_t>(m, JAICOV_NEWPT_MAX_RAYS);
            for (size_t j = 0; j < take; j++) {
                const Ray &r = rays[i][j * m / take];
                if (r.image->index < 0) continue;                      // an image the adjustment does not hold
                rayImage.push_back(r.image->index);
                xy.push_back(r.x); xy.push_back(r.y);
                disp.push_back(r.sx * r.sx); disp.push_back(r.sy * r.sy); disp.push_back(0.0);
            }
            rayBegin.push_back((int32_t)rayImage.size());
            start.push_back(fresh[i]->getX().getValue()); start.push_back(fresh[i]->getY().getValue()); start.push_back(fresh[i]->getZ().getValue());
        }
        if (fresh.size() >= 2) pairs = {0, 1};
        const BundleAdjustment::NewPoints r = ba.intersectNewPoints(s2, rayBegin, rayImage, xy, disp, start, pairs);
        size_t good = 0, larger = 0;
        std::printf("%-8s %4s %12s %12s %12s   %-26s   %-26s  status\n", "point", "rays", "X", "Y", "Z", "sigma from Q_meas alone", "sigma from Q_XX");
        for (size_t i = 0; i < fresh.size(); i++) {
            const double *o = &r.table[(size_t)JAICOV_NEWPT_COLUMNS * i];
            const double sm[3] = {std::sqrt(s2 * std::max(o[3], 0.0)), std::sqrt(s2 * std::max(o[6], 0.0)), std::sqrt(s2 * std::max(o[8], 0.0))};
            std::printf("%-8s %4d %12.4f %12.4f %12.4f   %8.5f %8.5f %8.5f   %8.5f %8.5f %8.5f  %d\n", fresh[i]->getName().c_str(),
                        rayBegin[i + 1] - rayBegin[i], o[0], o[1], o[2], sm[0], sm[1], sm[2], o[17], o[18], o[19], r.status[i]);
            if (r.status[i] & JAICOV_NEWPT_FAILED) continue;
            good++;
            if (o[17] >= sm[0] && o[18] >= sm[1] && o[19] >= sm[2]) larger++;
        }
        std::printf("new points intersected: %zu of %zu, sigma from Q_XX not below that from Q_meas: %zu\n", good, fresh.size(), larger);
        if (!pairs.empty()) {
            const double *l = r.lengths.data();
            std::printf("length %s - %s: L %.4f mm, sigma_L %.5f mm, q_L %.6e, without the correlations %.6e (status %d)\n",
                        fresh[0]->getName().c_str(), fresh[1]->getName().c_str(), l[0], l[1], l[5], l[6], r.lengthStatus[0]);
        }
        return good > 0 && larger == good ? 0 : 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 3;
    }
}
