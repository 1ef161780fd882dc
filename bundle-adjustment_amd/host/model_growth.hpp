// What example_relative and example_absolute share: a block's model grown from its image measurements and its camera alone.
//   1. the pair of images with the most common points is oriented relatively (RelativeOrientation::orientAll, base length 1);
//   2. every point that at least two oriented images see is intersected from those images (jaicov_isect_points);
//   3. every image not yet oriented that sees at least 6 intersected points is resected from them (jaicov_resect_images), and
//      where none does, every one that sees at least 4;
//   2 and 3 alternate until no image is added, then every point is intersected from all oriented images.
// Steps 2 and 3 call the C ABI with the oriented images' rays and the intersected points only; ForwardIntersection and SpatialResection
// take whole cameras.  The model lies in the frame of the pair's first image and its base length is 1.
#pragma once
#include <cstdio>
#include <limits>
#include <set>

#include "aicon_reader.hpp"

namespace jaicov::host::growth {

// points seen by at least two oriented images, from those images' rays; returns how many have coordinates afterwards
inline int intersect(Camera &cam, const std::set<Image *> &oriented, std::set<ObjectCoordinate *> &known) {
    std::vector<Image *> images(oriented.begin(), oriented.end());
    std::vector<ObjectCoordinate *> points;
    std::unordered_map<ObjectCoordinate *, size_t> indexOf;
    std::vector<std::vector<std::pair<int, ImageCoordinate *>>> rays;
    std::vector<double> io, eo;
    int n_images = 0;
    for (auto &im : cam.images()) {                                           // the camera's order, as ForwardIntersection takes it
        if (!oriented.count(im.get())) continue;
        for (int k = 0; k < 3; k++) io.push_back(cam.getInteriorOrientation().at(k)->getValue());
        for (int k = 0; k < 6; k++) eo.push_back(im->getExteriorOrientation().at(k)->getValue());
        for (auto &ic : im->coordinates()) {
            auto it = indexOf.find(ic->getObjectCoordinate());
            if (it == indexOf.end()) {
                it = indexOf.emplace(ic->getObjectCoordinate(), points.size()).first;
                points.push_back(ic->getObjectCoordinate());
                rays.emplace_back();
            }
            rays[it->second].push_back({n_images, ic.get()});
        }
        n_images++;
    }
    std::vector<int32_t> begin(1, 0), image;
    std::vector<double> xy, var;
    std::vector<ObjectCoordinate *> batch;
    for (size_t p = 0; p < points.size(); p++) {
        if (rays[p].size() < 2) continue;
        batch.push_back(points[p]);
        for (auto &r : rays[p]) {
            image.push_back(r.first);
            xy.push_back(r.second->getX().getValue()); xy.push_back(r.second->getY().getValue());
            var.push_back(r.second->getX().getVariance()); var.push_back(r.second->getY().getVariance());
            var.push_back(r.second->getCorrelationCoefficientXY());
        }
        begin.push_back((int32_t)image.size());
    }
    const int n = (int)batch.size();
    std::vector<double> out((size_t)JAICOV_ISECT_OUT_PER_POINT * n);
    std::vector<int32_t> status(n);
    const int rc = jaicov_isect_points(n, begin.data(), image.data(), xy.data(), var.data(), n_images, io.data(), eo.data(), 1.0, 50, 0.0, 2,
                                       out.data(), status.data(), nullptr, nullptr, nullptr, nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error("jaicov_isect_points failed with status " + std::to_string(rc));
    known.clear();
    for (int p = 0; p < n; p++) {
        if (status[p] != JAICOV_ISECT_OK) continue;
        const double *v = &out[(size_t)JAICOV_ISECT_OUT_PER_POINT * p];
        batch[p]->getX().setValue(v[0]); batch[p]->getY().setValue(v[1]); batch[p]->getZ().setValue(v[2]);
        known.insert(batch[p]);
    }
    return (int)known.size();
}

// images not yet oriented that see at least `least` known points, from those points; returns how many were added
inline int resect(Camera &cam, std::set<Image *> &oriented, const std::set<ObjectCoordinate *> &known, int least) {
    std::vector<Image *> images;
    std::vector<int32_t> begin(1, 0);
    std::vector<double> xy, xyz, var, io;
    for (auto &im : cam.images()) {
        if (oriented.count(im.get())) continue;
        int seen = 0;
        for (auto &ic : im->coordinates()) seen += (int)known.count(ic->getObjectCoordinate());
        if (seen < least) continue;
        images.push_back(im.get());
        for (int k = 0; k < 3; k++) io.push_back(cam.getInteriorOrientation().at(k)->getValue());
        for (auto &ic : im->coordinates()) {
            ObjectCoordinate *oc = ic->getObjectCoordinate();
            if (!known.count(oc)) continue;
            xy.push_back(ic->getX().getValue()); xy.push_back(ic->getY().getValue());
            xyz.push_back(oc->getX().getValue()); xyz.push_back(oc->getY().getValue()); xyz.push_back(oc->getZ().getValue());
            var.push_back(ic->getX().getVariance()); var.push_back(ic->getY().getVariance()); var.push_back(ic->getCorrelationCoefficientXY());
        }
        begin.push_back((int32_t)(xy.size() / 2));
    }
    const int n = (int)images.size();
    if (n == 0) return 0;
    std::vector<double> out((size_t)JAICOV_RESECT_OUT_PER_IMAGE * n);
    std::vector<int32_t> status(n);
    const int rc = jaicov_resect_images(n, begin.data(), xy.data(), xyz.data(), var.data(), io.data(), nullptr, 1.0, 50, 0.0, 4, out.data(),
                                        status.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != JAICOV_OK) throw std::runtime_error("jaicov_resect_images failed with status " + std::to_string(rc));
    int added = 0;
    for (int g = 0; g < n; g++) {
        if (status[g] != JAICOV_RESECT_OK) continue;
        for (int k = 0; k < 6; k++) images[g]->getExteriorOrientation().at(k)->setValue(out[(size_t)JAICOV_RESECT_OUT_PER_IMAGE * g + k]);
        oriented.insert(images[g]);
        added++;
    }
    return added;
}

// Steps 1 to 3 on a project whose camera is cam: the files' coordinates and orientations are forgotten, and the model of all images
// and points is built and reported line by line.  Throws where the block does not grow to all of its images and points.
inline void grow_model(AiconProject &pr, Camera &cam) {
    const double NaN = std::numeric_limits<double>::quiet_NaN();
    // nothing of object space is known: the files' coordinates and orientations are forgotten
    for (auto &p : pr.points) { p->getX().setValue(NaN); p->getY().setValue(NaN); p->getZ().setValue(NaN); }
    for (auto &im : cam.images())
        for (int k = 0; k < 6; k++) im->getExteriorOrientation().at(k)->setValue(NaN);

    // 1. the pair with the most common points (the first among equal counts, in the camera's order of images)
    Image *pa = nullptr, *pb = nullptr;
    size_t most = 0;
    {
        std::vector<std::set<ObjectCoordinate *>> sees;
        for (auto &im : cam.images()) {
            sees.emplace_back();
            for (auto &ic : im->coordinates()) sees.back().insert(ic->getObjectCoordinate());
        }
        for (size_t i = 0; i < sees.size(); i++)
            for (size_t j = i + 1; j < sees.size(); j++) {
                size_t common = 0;
                for (ObjectCoordinate *oc : sees[i]) common += sees[j].count(oc);
                if (common > most) { most = common; pa = cam.images()[i].get(); pb = cam.images()[j].get(); }
            }
    }
    if (!pa) throw std::runtime_error("no two images share a point");
    const std::vector<RelativeOrientation::Result> rel = RelativeOrientation::orientAll({{pa, pb}});
    const RelativeOrientation::Result &r = rel[0];
    std::printf("pair                          images %ld and %ld, %d common points\n", pa->getId(), pb->getId(), r.points);
    std::printf("relative orientation          status %d, start kind %d, %d Gauss-Newton steps, Omega %.6e\n", r.status, r.startKind,
                r.iterations, r.values[27]);
    if (!RelativeOrientation::apply(r, 1.0)) throw std::runtime_error("the relative orientation of the pair failed");

    // 2, 3. intersection and resection in alternation
    std::set<Image *> oriented = {pa, pb};
    std::set<ObjectCoordinate *> known;
    for (int round = 1;; round++) {
        const int np = intersect(cam, oriented, known);
        int added = resect(cam, oriented, known, 6);
        if (added == 0) added = resect(cam, oriented, known, 4);       // what is left sees few points: the plane start alone
        std::printf("round %-2d                      %d points intersected, %d images resected, %zu oriented\n", round, np, added, oriented.size());
        if (added == 0) break;
    }
    const int np = intersect(cam, oriented, known);
    std::printf("oriented images / points      %zu of %zu / %d of %zu\n", oriented.size(), cam.images().size(), np, pr.points.size());
    if (oriented.size() != cam.images().size() || (size_t)np != pr.points.size())
        throw std::runtime_error("the block did not grow to all of its images and points");
}

}  // namespace jaicov::host::growth
