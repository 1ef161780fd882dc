// pybind11 module _jaicov_host: exposes the C++ mirror of JAICOV's object API (jaicov.hpp) to the Python tests,
// examples and loaders.  Names follow the reference's Java API.
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "aicon_reader.hpp"
#include "result_writer.hpp"
#include "jaicov.hpp"

namespace py = pybind11;
using namespace jaicov::host;

PYBIND11_MODULE(_jaicov_host, m) {
    m.doc() = "C++ mirror of JAICOV's Camera/Image/ObjectCoordinate/BundleAdjustment API on the MI355X engine";
    m.attr("COLUMN_FIXED") = COLUMN_FIXED;
    m.attr("COLUMN_NOT_SET") = COLUMN_NOT_SET;

    py::enum_<ParameterType>(m, "ParameterType")
        .value("PRINCIPAL_POINT_X", ParameterType::PRINCIPAL_POINT_X).value("PRINCIPAL_POINT_Y", ParameterType::PRINCIPAL_POINT_Y)
        .value("PRINCIPAL_DISTANCE", ParameterType::PRINCIPAL_DISTANCE).value("RADIAL_POLYNOMIAL_A", ParameterType::RADIAL_POLYNOMIAL_A)
        .value("TANGENTIAL_POLYNOMIAL_B", ParameterType::TANGENTIAL_POLYNOMIAL_B)
        .value("TANGENTIAL_DISTORTION_Bx", ParameterType::TANGENTIAL_DISTORTION_Bx).value("TANGENTIAL_DISTORTION_By", ParameterType::TANGENTIAL_DISTORTION_By)
        .value("AFFINITY_AND_SHEAR_Cx", ParameterType::AFFINITY_AND_SHEAR_Cx).value("AFFINITY_AND_SHEAR_Cy", ParameterType::AFFINITY_AND_SHEAR_Cy)
        .value("DISTANCE_POLYNOMIAL_D", ParameterType::DISTANCE_POLYNOMIAL_D)
        .value("ZERNIKE_POLYNOMIAL_X", ParameterType::ZERNIKE_POLYNOMIAL_X).value("ZERNIKE_POLYNOMIAL_Y", ParameterType::ZERNIKE_POLYNOMIAL_Y)
        .value("ZERNIKE_POLYNOMIAL_Z", ParameterType::ZERNIKE_POLYNOMIAL_Z)
        .value("CAMERA_COORDINATE_X", ParameterType::CAMERA_COORDINATE_X).value("CAMERA_COORDINATE_Y", ParameterType::CAMERA_COORDINATE_Y)
        .value("CAMERA_COORDINATE_Z", ParameterType::CAMERA_COORDINATE_Z).value("CAMERA_OMEGA", ParameterType::CAMERA_OMEGA)
        .value("CAMERA_PHI", ParameterType::CAMERA_PHI).value("CAMERA_KAPPA", ParameterType::CAMERA_KAPPA)
        .value("OBJECT_COORDINATE_X", ParameterType::OBJECT_COORDINATE_X).value("OBJECT_COORDINATE_Y", ParameterType::OBJECT_COORDINATE_Y)
        .value("OBJECT_COORDINATE_Z", ParameterType::OBJECT_COORDINATE_Z);
    py::enum_<EstimationStateType>(m, "EstimationStateType")
        .value("ERROR_FREE_ESTIMATION", EstimationStateType::ERROR_FREE_ESTIMATION).value("BUSY", EstimationStateType::BUSY)
        .value("INTERRUPT", EstimationStateType::INTERRUPT).value("SINGULAR_MATRIX", EstimationStateType::SINGULAR_MATRIX)
        .value("NO_CONVERGENCE", EstimationStateType::NO_CONVERGENCE).value("NOT_INITIALISED", EstimationStateType::NOT_INITIALISED)
        .value("ROBUST_ESTIMATION_FAILED", EstimationStateType::ROBUST_ESTIMATION_FAILED)
        .value("EXPORT_ADJUSTMENT_RESULTS_FAILED", EstimationStateType::EXPORT_ADJUSTMENT_RESULTS_FAILED)
        .value("OUT_OF_MEMORY", EstimationStateType::OUT_OF_MEMORY);
    py::enum_<EstimationType>(m, "EstimationType").value("L2NORM", EstimationType::L2NORM).value("SIMULATION", EstimationType::SIMULATION);
    py::enum_<MatrixInversion>(m, "MatrixInversion")
        .value("NONE", MatrixInversion::NONE).value("FULL", MatrixInversion::FULL)
        .value("PRE_ELIMINATION", MatrixInversion::PRE_ELIMINATION).value("REDUCED", MatrixInversion::REDUCED);
    py::enum_<DistortionModel::Type>(m, "DistortionModelType")
        .value("AFFINITY_AND_SHEAR", DistortionModel::Type::AFFINITY_AND_SHEAR).value("TANGENTIAL_DISTORTION", DistortionModel::Type::TANGENTIAL_DISTORTION)
        .value("RADIAL_DISTORTION", DistortionModel::Type::RADIAL_DISTORTION).value("DISTANCE_DISTORTION", DistortionModel::Type::DISTANCE_DISTORTION)
        .value("ZERNIKE_X", DistortionModel::Type::ZERNIKE_X).value("ZERNIKE_Y", DistortionModel::Type::ZERNIKE_Y)
        .value("ZERNIKE_GRADIENT", DistortionModel::Type::ZERNIKE_GRADIENT);

    py::class_<UnknownParameter>(m, "UnknownParameter")
        .def("getParameterType", &UnknownParameter::getParameterType)
        .def("getValue", &UnknownParameter::getValue).def("setValue", &UnknownParameter::setValue)
        .def("getColumn", &UnknownParameter::getColumn).def("setColumn", &UnknownParameter::setColumn)
        .def("getOrder", &UnknownParameter::getOrder);
    py::class_<ObservationParameter>(m, "ObservationParameter")
        .def(py::init<UnknownParameter *>(), py::keep_alive<1, 2>())
        .def("getValue", &ObservationParameter::getValue).def("setValue", &ObservationParameter::setValue)
        .def("getVariance", &ObservationParameter::getVariance).def("setVariance", &ObservationParameter::setVariance)
        .def("getRow", &ObservationParameter::getRow);
    py::class_<ObjectCoordinate>(m, "ObjectCoordinate")
        .def(py::init<std::string, double, double, double>())
        .def("getName", &ObjectCoordinate::getName)
        .def("getX", &ObjectCoordinate::getX, py::return_value_policy::reference_internal)
        .def("getY", &ObjectCoordinate::getY, py::return_value_policy::reference_internal)
        .def("getZ", &ObjectCoordinate::getZ, py::return_value_policy::reference_internal)
        .def("isDatum", &ObjectCoordinate::isDatum).def("setDatum", &ObjectCoordinate::setDatum);
    py::class_<ScaleBar>(m, "ScaleBar")
        .def(py::init<ObjectCoordinate *, ObjectCoordinate *, double, double>(), py::keep_alive<1, 2>(), py::keep_alive<1, 3>())
        .def("getLength", &ScaleBar::getLength, py::return_value_policy::reference_internal);
    py::class_<DistortionModel>(m, "DistortionModel")
        .def("getType", &DistortionModel::getType).def("getR0", &DistortionModel::getR0)
        .def("add", &DistortionModel::add, py::return_value_policy::reference_internal)
        .def("get", &DistortionModel::get, py::return_value_policy::reference_internal)
        .def("getCx", &DistortionModel::getCx, py::return_value_policy::reference_internal)
        .def("getCy", &DistortionModel::getCy, py::return_value_policy::reference_internal)
        .def("getBx", &DistortionModel::getBx, py::return_value_policy::reference_internal)
        .def("getBy", &DistortionModel::getBy, py::return_value_policy::reference_internal)
        .def("parameters", [](DistortionModel &d) {
            std::vector<UnknownParameter *> v;
            for (auto &p : d.parameters()) v.push_back(p.get());
            return v;
        }, py::return_value_policy::reference_internal);
    py::class_<InteriorOrientation>(m, "InteriorOrientation")
        .def("getPrinciplePointX", &InteriorOrientation::getPrinciplePointX, py::return_value_policy::reference_internal)
        .def("getPrinciplePointY", &InteriorOrientation::getPrinciplePointY, py::return_value_policy::reference_internal)
        .def("getPrincipleDistance", &InteriorOrientation::getPrincipleDistance, py::return_value_policy::reference_internal);
    py::class_<ExteriorOrientation>(m, "ExteriorOrientation")
        .def("get", &ExteriorOrientation::get, py::return_value_policy::reference_internal);
    py::class_<ImageCoordinate>(m, "ImageCoordinate")
        .def("getObjectCoordinate", &ImageCoordinate::getObjectCoordinate, py::return_value_policy::reference)
        .def("getX", &ImageCoordinate::getX, py::return_value_policy::reference_internal)
        .def("getY", &ImageCoordinate::getY, py::return_value_policy::reference_internal)
        .def("getCorrelationCoefficientXY", &ImageCoordinate::getCorrelationCoefficientXY);
    py::class_<Image>(m, "Image")
        .def("getId", &Image::getId)
        .def("getExteriorOrientation", &Image::getExteriorOrientation, py::return_value_policy::reference_internal)
        .def("add", &Image::add, py::return_value_policy::reference_internal, py::keep_alive<1, 2>(), py::arg("objectCoordinate"),
             py::arg("xp"), py::arg("yp"), py::arg("sigmax"), py::arg("sigmay"), py::arg("corrCoefXY") = 0.0)
        .def("getNumberOfImageCoordinates", &Image::getNumberOfImageCoordinates)
        .def("setDispersion", [](Image &im, py::array_t<double, py::array::c_style | py::array::forcecast> D) {
            im.setDispersion(std::vector<double>(D.data(), D.data() + D.size()));
        })
        .def("coordinates", [](Image &im) {
            std::vector<ImageCoordinate *> v;
            for (auto &c : im.coordinates()) v.push_back(c.get());
            return v;
        }, py::return_value_policy::reference_internal);
    py::class_<Camera>(m, "Camera")
        .def(py::init<long, double, std::vector<DistortionModel::Type>>())
        .def("getId", &Camera::getId)
        .def("getInteriorOrientation", &Camera::getInteriorOrientation, py::return_value_policy::reference_internal)
        .def("add", &Camera::add, py::return_value_policy::reference_internal)
        .def("getNumberOfImages", &Camera::getNumberOfImages)
        .def("getDistortionModel", &Camera::getDistortionModel, py::return_value_policy::reference_internal)
        .def("images", [](Camera &c) {
            std::vector<Image *> v;
            for (auto &im : c.images()) v.push_back(im.get());
            return v;
        }, py::return_value_policy::reference_internal);
    py::class_<DirectlyObservedParameterGroup>(m, "DirectlyObservedParameterGroup")
        .def(py::init<std::vector<ObservationParameter *>>(), py::keep_alive<1, 2>())
        .def(py::init([](py::array_t<double, py::array::c_style | py::array::forcecast> D, std::vector<ObservationParameter *> obs) {
                 return new DirectlyObservedParameterGroup(std::vector<double>(D.data(), D.data() + D.size()), std::move(obs));
             }), py::keep_alive<1, 3>())
        .def("hasFullyPopulatedWeightMatrix", &DirectlyObservedParameterGroup::hasFullyPopulatedWeightMatrix)
        .def("getNumberOfParameters", &DirectlyObservedParameterGroup::getNumberOfParameters);

    py::class_<BundleAdjustment>(m, "BundleAdjustment")
        .def(py::init<>())
        .def("add", py::overload_cast<Camera *>(&BundleAdjustment::add), py::keep_alive<1, 2>())
        .def("add", py::overload_cast<ScaleBar *>(&BundleAdjustment::add), py::keep_alive<1, 2>())
        .def("add", py::overload_cast<DirectlyObservedParameterGroup *>(&BundleAdjustment::add), py::keep_alive<1, 2>())
        .def("addPropertyChangeListener", &BundleAdjustment::addPropertyChangeListener)
        .def("setEstimationType", &BundleAdjustment::setEstimationType)
        .def("setInvertNormalEquation", &BundleAdjustment::setInvertNormalEquation)
        .def("setAdjustmentResultWriter", &BundleAdjustment::setAdjustmentResultWriter, py::keep_alive<1, 2>())
        .def("hasCofactorMatrix", &BundleAdjustment::hasCofactorMatrix)
        .def("cofactorSub", [](BundleAdjustment &b, std::vector<int32_t> idx, double scale) {
            std::vector<double> v = b.cofactorSub(idx, scale);
            return py::array_t<double>({idx.size(), idx.size()}, v.data());
        }, py::arg("indices"), py::arg("scale") = 1.0)
        .def("observationReliability", [](BundleAdjustment &b, double sigma2Test) {
            auto o = b.observationReliability(sigma2Test);
            auto arr = [](const std::vector<double> &x) { return py::array_t<double>((py::ssize_t)x.size(), x.data()); };
            return py::make_tuple(arr(o.v), arr(o.qvv), arr(o.r), arr(o.t));
        }, py::arg("sigma2Test"), "(v, qvv, r, t) of every observation row (include/jaicov_reliability.h)")
        .def("imagePointReliability", [](BundleAdjustment &b, double sigma2Test, double lambda0) {
            auto o = b.imagePointReliability(sigma2Test, lambda0);
            auto arr = [](const std::vector<double> &x) { return py::array_t<double>((py::ssize_t)x.size(), x.data()); };
            return py::make_tuple(arr(o.q), arr(o.Tprio), arr(o.Tpost), arr(o.nablaX), arr(o.nablaY), arr(o.Mxx), arr(o.Mxy), arr(o.Myy),
                                  arr(o.mdbMajor), arr(o.mdbMinor), arr(o.deltaExt), arr(o.dX), arr(o.dY), arr(o.dZ));
        }, py::arg("sigma2Test"), py::arg("lambda0") = 17.075,
             "(q, T_prio, T_post, nabla_x, nabla_y, Mxx, Mxy, Myy, mdb_major, mdb_minor, delta_ext, dX, dY, dZ) of every image point "
             "(include/jaicov_reliability_points.h)")
        .def("transformDatum", &BundleAdjustment::transformDatum,
             "re-express the cofactor matrix in the datum of the points flagged now (include/jaicov_datum.h)")
        .def("pointPrecision", [](BundleAdjustment &b, double sigma2, double k3, double k2, std::vector<int32_t> points) {
            auto t = b.pointPrecision(sigma2, k3, k2, points);
            return py::make_tuple(py::array_t<double>({t.status.size(), (size_t)t.columns}, t.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)t.status.size(), t.status.data()));
        }, py::arg("sigma2"), py::arg("k3") = 1.0, py::arg("k2") = 1.0, py::arg("points") = std::vector<int32_t>(),
             "(table (n, 22), status (n,)) of the object points (include/jaicov_precision.h); no points = all")
        .def("stationPrecision", [](BundleAdjustment &b, double sigma2, double k3, double k2, std::vector<int32_t> images) {
            auto t = b.stationPrecision(sigma2, k3, k2, images);
            return py::make_tuple(py::array_t<double>({t.status.size(), (size_t)t.columns}, t.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)t.status.size(), t.status.data()));
        }, py::arg("sigma2"), py::arg("k3") = 1.0, py::arg("k2") = 1.0, py::arg("images") = std::vector<int32_t>(),
             "(table (n, 25), status (n,)) of the projection centres (include/jaicov_precision.h); no images = all")
        .def("lengthPrecision", [](BundleAdjustment &b, double sigma2, std::vector<int32_t> pairs) {
            auto t = b.lengthPrecision(sigma2, pairs);
            return py::make_tuple(py::array_t<double>({t.status.size(), (size_t)t.columns}, t.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)t.status.size(), t.status.data()));
        }, py::arg("sigma2"), py::arg("pairs"), "(table (n, 5), status (n,)) of the lengths between the point pairs (A, B), flattened")
        .def("principalComponents", [](BundleAdjustment &b, int firstCol, int nCols, int k, double tol, int maxIterations) {
            auto c = b.principalComponents(firstCol, nCols, k, tol, maxIterations);
            return py::make_tuple(py::array_t<double>((py::ssize_t)c.values.size(), c.values.data()),
                                  py::array_t<double>({c.values.size(), (size_t)std::max(nCols, 0)}, c.vectors.data()), c.trace,
                                  py::array_t<double>((py::ssize_t)c.residuals.size(), c.residuals.data()), c.iterations, c.converged);
        }, py::arg("firstCol"), py::arg("nCols"), py::arg("k"), py::arg("tol") = 0.0, py::arg("maxIterations") = 200,
             "(values, vectors (k, nCols), trace, residuals, iterations, converged) of the sub-block's largest eigenpairs")
        .def("parameterCorrelations", [](BundleAdjustment &b, uint32_t pairMask, uint32_t flags) {
            auto c = b.parameterCorrelations(pairMask, flags);
            return py::make_tuple(py::array_t<double>((py::ssize_t)c.rho.size(), c.rho.data()),
                                  py::array_t<int32_t>((py::ssize_t)c.partner.size(), c.partner.data()),
                                  py::array_t<int32_t>((py::ssize_t)c.status.size(), c.status.data()));
        }, py::arg("pairMask") = 0xFFFFu, py::arg("flags") = 0u,
             "(rho, partner, status) of every column: its worst-correlated admissible partner (include/jaicov_parameters.h)")
        .def("correlatedPairs", [](BundleAdjustment &b, double threshold, uint32_t pairMask, uint32_t flags, int64_t capacity) {
            auto p = b.correlatedPairs(threshold, pairMask, flags, capacity);
            return py::make_tuple(py::array_t<int32_t>({p.rho.size(), (size_t)2}, p.cols.data()),
                                  py::array_t<double>((py::ssize_t)p.rho.size(), p.rho.data()), p.count);
        }, py::arg("threshold"), py::arg("pairMask") = 0xFFFFu, py::arg("flags") = 0u, py::arg("capacity") = (int64_t)1 << 16,
             "(cols (m, 2), rho (m,), count) of the pairs with |rho| >= threshold, sorted; empty when count exceeds the capacity")
        .def("correlationBlock", [](BundleAdjustment &b, std::vector<int32_t> rowCols, std::vector<int32_t> colCols) {
            auto o = b.correlationBlock(rowCols, colCols);
            return py::array_t<double>({rowCols.size(), colCols.size()}, o.data());
        }, py::arg("rowCols"), py::arg("colCols"), "rho between two lists of columns, (n_r, n_c)")
        .def("testParameters", [](BundleAdjustment &b, double sigma2, std::vector<int32_t> groupBegin, std::vector<int32_t> groupSlot,
                                  std::vector<double> x0) {
            auto t = b.testParameters(sigma2, groupBegin, groupSlot, x0);
            return py::make_tuple(py::array_t<double>({t.status.size(), (size_t)JAICOV_PAR_TEST_COLUMNS}, t.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)t.status.size(), t.status.data()));
        }, py::arg("sigma2"), py::arg("groupBegin"), py::arg("groupSlot"), py::arg("x0") = std::vector<double>(),
             "(table (n, 4): q, T, k, t; status (n,)) of the test x_g = x0_g on groups of slots (include/jaicov_parameters.h)")
        .def("fitForms", [](BundleAdjustment &b, double sigma2, std::vector<int32_t> formType, std::vector<int32_t> formBegin,
                            std::vector<int32_t> formPoint, int maxIterations, double tol) {
            auto f = b.fitForms(sigma2, formType, formBegin, formPoint, maxIterations, tol);
            return py::make_tuple(py::array_t<double>({f.status.size(), (size_t)JAICOV_FORM_COLUMNS}, f.table.data()),
                                  py::array_t<double>({f.status.size(), (size_t)JAICOV_FORM_QPP_COLUMNS}, f.qpp.data()),
                                  py::array_t<double>({f.memberStatus.size(), (size_t)JAICOV_FORM_MEMBER_COLUMNS}, f.members.data()),
                                  py::array_t<int32_t>((py::ssize_t)f.status.size(), f.status.data()),
                                  py::array_t<int32_t>((py::ssize_t)f.memberStatus.size(), f.memberStatus.data()));
        }, py::arg("sigma2"), py::arg("formType"), py::arg("formBegin"), py::arg("formPoint"), py::arg("maxIterations") = 20, py::arg("tol") = 0.0,
             "(table (n, 20), qpp (n, 28), members (M, 7), status (n,), member status (M,)) of the forms through object points (include/jaicov_forms.h)")
        .def("fitSurfaces", [](BundleAdjustment &b, double sigma2, std::vector<int32_t> formType, std::vector<int32_t> formBegin,
                               std::vector<int32_t> formPoint, std::vector<double> start, int maxIterations, double tol) {
            auto f = b.fitSurfaces(sigma2, formType, formBegin, formPoint, start, maxIterations, tol);
            return py::make_tuple(py::array_t<double>({f.status.size(), (size_t)JAICOV_FORM_COLUMNS}, f.table.data()),
                                  py::array_t<double>({f.status.size(), (size_t)JAICOV_FORM_QPP_COLUMNS}, f.qpp.data()),
                                  py::array_t<double>({f.memberStatus.size(), (size_t)JAICOV_FORM_MEMBER_COLUMNS}, f.members.data()),
                                  py::array_t<int32_t>((py::ssize_t)f.status.size(), f.status.data()),
                                  py::array_t<int32_t>((py::ssize_t)f.memberStatus.size(), f.memberStatus.data()));
        }, py::arg("sigma2"), py::arg("formType"), py::arg("formBegin"), py::arg("formPoint"), py::arg("start") = std::vector<double>(),
             py::arg("maxIterations") = 20, py::arg("tol") = 0.0,
             "the tuple of fitForms for the types 0 .. 5 (cylinders and cones), with start values (n x 7, flat) or none (include/jaicov_surfaces.h)")
        .def("predictImagePoints", [](BundleAdjustment &b, double sigma2, std::vector<int32_t> images, std::vector<int32_t> points, double k2) {
            auto t = b.predictImagePoints(sigma2, images, points, k2);
            return py::make_tuple(py::array_t<double>({t.status.size(), (size_t)t.columns}, t.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)t.status.size(), t.status.data()));
        }, py::arg("sigma2"), py::arg("images"), py::arg("points"), py::arg("k2") = 1.0,
             "(table (n, 10), status (n,)) of the predicted image points of the pairs (image, point) (include/jaicov_predict.h)")
        .def("checkImagePoints", [](BundleAdjustment &b, std::vector<int32_t> images, std::vector<int32_t> points, std::vector<double> xy,
                                    std::vector<double> disp, double sigma2Post, std::vector<int32_t> groupBegin) {
            auto c = b.checkImagePoints(images, points, xy, disp, sigma2Post, groupBegin);
            return py::make_tuple(py::array_t<double>({c.status.size(), (size_t)JAICOV_PRED_CHECK_COLUMNS}, c.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)c.status.size(), c.status.data()),
                                  py::array_t<double>({c.groupStatus.size(), (size_t)JAICOV_PRED_GROUP_COLUMNS}, c.groups.data()),
                                  py::array_t<int32_t>((py::ssize_t)c.groupStatus.size(), c.groupStatus.data()));
        }, py::arg("images"), py::arg("points"), py::arg("xy"), py::arg("disp"), py::arg("sigma2Post") = 0.0, py::arg("groupBegin") = std::vector<int32_t>(),
             "(table (n, 8), status (n,), groups (G, 4), group status (G,)) of the test of check measurements (include/jaicov_predict.h)")
        .def("intersectNewPoints", [](BundleAdjustment &b, double sigma2, std::vector<int32_t> rayBegin, std::vector<int32_t> rayImage,
                                      std::vector<double> xy, std::vector<double> disp, std::vector<double> start, std::vector<int32_t> pairs,
                                      int maxIterations) {
            auto r = b.intersectNewPoints(sigma2, rayBegin, rayImage, xy, disp, start, pairs, maxIterations);
            return py::make_tuple(py::array_t<double>({r.status.size(), (size_t)JAICOV_NEWPT_COLUMNS}, r.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)r.status.size(), r.status.data()),
                                  py::array_t<int32_t>((py::ssize_t)r.iterations.size(), r.iterations.data()),
                                  py::array_t<double>({r.rayW.size() / 2, (size_t)2}, r.rayW.data()),
                                  py::array_t<double>({r.lengthStatus.size(), (size_t)JAICOV_NEWPT_PAIR_COLUMNS}, r.lengths.data()),
                                  py::array_t<int32_t>((py::ssize_t)r.lengthStatus.size(), r.lengthStatus.data()));
        }, py::arg("sigma2"), py::arg("rayBegin"), py::arg("rayImage"), py::arg("xy"), py::arg("disp"), py::arg("start"),
             py::arg("pairs") = std::vector<int32_t>(), py::arg("maxIterations") = 20,
             "(table (n, 20), status (n,), iterations (n,), ray_w (R, 2), lengths (G, 7), length status (G,)) of new object points (include/jaicov_newpoints.h)")
        .def("varianceComponents", [](BundleAdjustment &b, std::vector<int32_t> ip, std::vector<int32_t> sb, std::vector<int32_t> dg, int nGroups,
                                      double sigma2Test) {
            BundleAdjustment::VarianceGroups g;
            g.ip = std::move(ip); g.sb = std::move(sb); g.dg = std::move(dg); g.nGroups = nGroups;
            auto r = b.varianceComponents(g, sigma2Test);
            const double summary[5] = {r.omega, r.sumR, r.rowsGrouped, r.rowsUngrouped, r.damping};
            return py::make_tuple(py::array_t<double>({(size_t)JAICOV_VCE_COLUMNS, r.status.size()}, r.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)r.status.size(), r.status.data()), py::array_t<double>(5, summary));
        }, py::arg("ip") = std::vector<int32_t>(), py::arg("sb") = std::vector<int32_t>(), py::arg("dg") = std::vector<int32_t>(),
             py::arg("nGroups") = 0, py::arg("sigma2Test") = 0.0,
             "(table (6, G), status (G,), summary (5,)) of the variance components of groups of observations (include/jaicov_vce.h)")
        .def("calibrationField", [](BundleAdjustment &b, double sigma2, std::vector<int32_t> cameras, std::vector<double> xy, std::vector<double> depth,
                                    double k2, uint32_t columns, bool withJacobian) {
            auto f = b.calibrationField(sigma2, cameras, xy, depth, k2, columns, withJacobian);
            const size_t n = f.status.size();
            return py::make_tuple(py::array_t<double>({n, (size_t)JAICOV_CALIB_FIELD_COLUMNS}, f.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)n, f.status.data()),
                                  py::array_t<double>({withJacobian ? n : (size_t)0, (size_t)2, (size_t)JAICOV_CALIB_MAX_COLUMNS}, f.jacobian.data()));
        }, py::arg("sigma2"), py::arg("cameras"), py::arg("xy"), py::arg("depth") = std::vector<double>(), py::arg("k2") = 1.0,
             py::arg("columns") = (uint32_t)JAICOV_CALIB_ALL, py::arg("withJacobian") = false,
             "(table (n, 14), status (n,), jacobian (n, 2, 23) or (0, 2, 23)) of the distortion field at the nodes (include/jaicov_calibration.h)")
        .def("compareCalibration", [](BundleAdjustment &b, int camA, int camB, std::vector<double> xy, std::vector<double> depth,
                                      std::vector<double> refValues, std::vector<double> refCov, double sigma2Post, bool relative) {
            auto c = b.compareCalibration(camA, camB, xy, depth, refValues, refCov, sigma2Post, relative);
            const size_t n = c.status.size();
            return py::make_tuple(py::array_t<double>({n, (size_t)JAICOV_CALIB_COMPARE_COLUMNS}, c.table.data()),
                                  py::array_t<int32_t>((py::ssize_t)n, c.status.data()),
                                  py::array_t<double>((py::ssize_t)JAICOV_CALIB_SUMMARY_COLUMNS, c.summary));
        }, py::arg("camA"), py::arg("camB"), py::arg("xy"), py::arg("depth") = std::vector<double>(), py::arg("refValues") = std::vector<double>(),
             py::arg("refCov") = std::vector<double>(), py::arg("sigma2Post") = 0.0, py::arg("relative") = false,
             "(table (n, 8), status (n,), summary (8,)) of the difference field of two calibrations (include/jaicov_calibration.h)")
        .def("cameraValues", &BundleAdjustment::cameraValues, "x0, y0, c and the coefficients of a camera at the engine's current values")
        .def("useCentroidedCoordinates", &BundleAdjustment::useCentroidedCoordinates)
        .def("centroidCoordinates", &BundleAdjustment::centroidCoordinates)
        .def("applyAposterioriVarianceOfUnitWeight", &BundleAdjustment::applyAposterioriVarianceOfUnitWeight)
        .def("setLevenbergMarquardtDampingValue", &BundleAdjustment::setLevenbergMarquardtDampingValue)
        .def("setMaximalNumberOfIterations", &BundleAdjustment::setMaximalNumberOfIterations)
        .def("setDevice", &BundleAdjustment::setDevice)
        .def("prepareUnknownParameters", &BundleAdjustment::prepareUnknownParameters)
        .def("flatten", &BundleAdjustment::flatten)
        .def("estimateModel", &BundleAdjustment::estimateModel, py::call_guard<py::gil_scoped_release>())
        .def("getNumberOfObservations", &BundleAdjustment::getNumberOfObservations)
        .def("getNumberOfUnknownParameters", &BundleAdjustment::getNumberOfUnknownParameters)
        .def("getNumberOfDatumConditions", &BundleAdjustment::getNumberOfDatumConditions)
        .def("getDegreeOfFreedom", &BundleAdjustment::getDegreeOfFreedom)
        .def("getVarianceFactorApriori", &BundleAdjustment::getVarianceFactorApriori)
        .def("getVarianceFactorAposteriori", &BundleAdjustment::getVarianceFactorAposteriori)
        .def("getOmega", &BundleAdjustment::getOmega)
        .def("getIterations", &BundleAdjustment::getIterations)
        .def("getDatumFlags", [](BundleAdjustment &b) { return b.getRankDefect().flags(); })
        .def("lastError", &BundleAdjustment::lastError)
        .def("nativeEngineHandle", [](BundleAdjustment &b) { return (uintptr_t)b.nativeEngine(); })
        .def("getObjectCoordinates", [](BundleAdjustment &b) { return b.getObjectCoordinates(); }, py::return_value_policy::reference_internal)
        .def("getCofactorMatrix", [](BundleAdjustment &b) {
            const auto &q = b.getCofactorMatrix();
            return py::array_t<double>(q.size(), q.data());
        })
        .def("flat", [](BundleAdjustment &b) {
            // the flattened arrays as a dict of numpy arrays (parity tests feed them to the oracle)
            py::dict d;
            const auto &f = b.flat;
            auto I = [](const std::vector<int32_t> &v) { return py::array_t<int32_t>(v.size(), v.data()); };
            auto D = [](const std::vector<double> &v) { return py::array_t<double>(v.size(), v.data()); };
            auto L = [](const std::vector<int64_t> &v) { return py::array_t<int64_t>(v.size(), v.data()); };
            d["point_col"] = I(f.point_col); d["io_col"] = I(f.io_col); d["cam_dist_begin"] = I(f.cam_dist_begin);
            d["dist_kind"] = I(f.dist_kind); d["dist_order"] = I(f.dist_order); d["dist_col"] = I(f.dist_col);
            d["image_camera"] = I(f.image_camera); d["eo_col"] = I(f.eo_col); d["ip_image"] = I(f.ip_image); d["ip_point"] = I(f.ip_point);
            d["blk_ip_begin"] = I(f.blk_ip_begin); d["sb_point_a"] = I(f.sb_a); d["sb_point_b"] = I(f.sb_b);
            d["dg_row_begin"] = I(f.dg_row_begin); d["dg_slot"] = I(f.dg_slot);
            d["point_datum"] = py::array_t<uint8_t>(f.point_datum.size(), f.point_datum.data());
            d["cam_r0"] = D(f.cam_r0); d["ip_x"] = D(f.ip_x); d["ip_y"] = D(f.ip_y); d["ip_var_x"] = D(f.ip_var_x); d["ip_var_y"] = D(f.ip_var_y);
            d["ip_rho"] = D(f.ip_rho); d["blk_disp"] = D(f.blk_disp); d["sb_length"] = D(f.sb_len); d["sb_var"] = D(f.sb_var);
            d["dg_obs"] = D(f.dg_obs); d["dg_var"] = D(f.dg_var); d["dg_disp"] = D(f.dg_disp); d["values"] = D(f.values);
            d["blk_disp_offset"] = L(f.blk_disp_offset); d["dg_disp_offset"] = L(f.dg_disp_offset);
            d["n_unknowns"] = b.getNumberOfUnknownParameters() + b.getNumberOfDatumConditions();
            d["rank_defect"] = b.getNumberOfDatumConditions();
            d["datum_flags"] = b.getRankDefect().flags();
            d["sigma2apriori"] = b.getVarianceFactorApriori();
            return d;
        });

    py::class_<AdjustmentResultWritable>(m, "AdjustmentResultWritable")
        .def("export", &AdjustmentResultWritable::exportResults);
    py::class_<DefaultResultWriter, AdjustmentResultWritable>(m, "DefaultResultWriter")
        .def(py::init<std::string>())
        .def("toString", &DefaultResultWriter::toString);
    py::class_<MatlabResultWriter, AdjustmentResultWritable>(m, "MatlabResultWriter")
        .def(py::init<std::string>())
        .def("toString", &MatlabResultWriter::toString);
    m.def("java_fixed", &java_fixed, "java.util.Formatter %[+].<prec>f");

    py::class_<CoordinateTransformationExteriorOrientation, std::unique_ptr<CoordinateTransformationExteriorOrientation, py::nodelete>>(
        m, "CoordinateTransformationExteriorOrientation")
        .def_static("getInstance", &CoordinateTransformationExteriorOrientation::getInstance, py::return_value_policy::reference)
        .def("transform", &CoordinateTransformationExteriorOrientation::transform, py::arg("objectCoordinatesToTransform"),
             py::arg("imagesToAlign"), py::arg("sigma2"), py::arg("adjustment"), py::call_guard<py::gil_scoped_release>())
        .def("getCovarianceMatrix", [](const CoordinateTransformationExteriorOrientation &t) {
            const auto &v = t.getCovarianceMatrix();
            return py::array_t<double>((py::ssize_t)v.size(), v.data());
        })
        .def("getTransformedCoordinates", &CoordinateTransformationExteriorOrientation::getTransformedCoordinates,
             py::return_value_policy::reference);

    py::class_<DLTCoefficients>(m, "DLTCoefficients")
        .def(py::init<Image *>(), py::keep_alive<1, 2>())
        .def("get", &DLTCoefficients::get, py::return_value_policy::reference_internal)
        .def("getReference", &DLTCoefficients::getReference, py::return_value_policy::reference)
        .def("values", [](DLTCoefficients &c) {
            std::vector<double> v;
            for (int k = 0; k < 20; k++) v.push_back(c.at(k)->getValue());
            return v;
        })
        .def_readonly("status", &DLTCoefficients::status)
        .def_readonly("solves", &DLTCoefficients::solves);
    py::class_<DirectLinearTransformation> dlt(m, "DirectLinearTransformation");
    py::enum_<DirectLinearTransformation::RestrictionType>(dlt, "RestrictionType")
        .value("IDENTICAL_PRINCIPLE_DISTANCE", DirectLinearTransformation::RestrictionType::IDENTICAL_PRINCIPLE_DISTANCE)
        .value("ROTATION_WITHOUT_SHEAR", DirectLinearTransformation::RestrictionType::ROTATION_WITHOUT_SHEAR)
        .value("FIXED_PRINCIPLE_DISTANCE_X", DirectLinearTransformation::RestrictionType::FIXED_PRINCIPLE_DISTANCE_X)
        .value("FIXED_PRINCIPLE_DISTANCE_Y", DirectLinearTransformation::RestrictionType::FIXED_PRINCIPLE_DISTANCE_Y)
        .value("FIXED_PRINCIPAL_POINT_X", DirectLinearTransformation::RestrictionType::FIXED_PRINCIPAL_POINT_X)
        .value("FIXED_PRINCIPAL_POINT_Y", DirectLinearTransformation::RestrictionType::FIXED_PRINCIPAL_POINT_Y);
    dlt.def_static("adjust", [](DLTCoefficients &c, AiconProject &pr, std::vector<DirectLinearTransformation::RestrictionType> rs) {
           return DirectLinearTransformation::adjust(c, pr.byName, rs);
       }, py::arg("coefficients"), py::arg("project"), py::arg("restrictions") = std::vector<DirectLinearTransformation::RestrictionType>{})
        .def_static("adjustAll", [](std::vector<DLTCoefficients *> cs, AiconProject &pr, std::vector<DirectLinearTransformation::RestrictionType> rs) {
           return DirectLinearTransformation::adjustAll(cs, pr.byName, rs);
       }, py::arg("coefficients"), py::arg("project"), py::arg("restrictions") = std::vector<DirectLinearTransformation::RestrictionType>{})
        .def_static("applyExteriorOrientation", &DirectLinearTransformation::applyExteriorOrientation)
        .def_static("setMaximalNumberOfIterations", &DirectLinearTransformation::setMaximalNumberOfIterations);

    py::class_<ForwardIntersection> isect(m, "ForwardIntersection");
    py::class_<ForwardIntersection::Result>(isect, "Result")
        .def_property_readonly("point", [](ForwardIntersection::Result &r) { return r.point; }, py::return_value_policy::reference)
        .def_readonly("status", &ForwardIntersection::Result::status)
        .def_readonly("iterations", &ForwardIntersection::Result::iterations)
        .def_readonly("rays", &ForwardIntersection::Result::rays)
        .def_readonly("raysUsed", &ForwardIntersection::Result::raysUsed)
        .def("values", [](ForwardIntersection::Result &r) { return std::vector<double>(r.values, r.values + JAICOV_ISECT_OUT_PER_POINT); });
    isect.def_static("intersectAll", &ForwardIntersection::intersectAll, py::arg("cameras"), py::arg("sigma2apriori") = 1.0,
                     py::arg("rejectThreshold") = 0.0, py::arg("minRays") = 3, py::return_value_policy::move)
        .def_static("setMaximalNumberOfIterations", &ForwardIntersection::setMaximalNumberOfIterations);
    py::class_<SpatialResection> resect(m, "SpatialResection");
    py::class_<SpatialResection::Result>(resect, "Result")
        .def_property_readonly("image", [](SpatialResection::Result &r) { return r.image; }, py::return_value_policy::reference)
        .def_readonly("status", &SpatialResection::Result::status)
        .def_readonly("iterations", &SpatialResection::Result::iterations)
        .def_readonly("startKind", &SpatialResection::Result::startKind)
        .def_readonly("points", &SpatialResection::Result::points)
        .def_readonly("pointsUsed", &SpatialResection::Result::pointsUsed)
        .def("values", [](SpatialResection::Result &r) { return std::vector<double>(r.values, r.values + JAICOV_RESECT_OUT_PER_IMAGE); });
    resect.def_static("resectAll", &SpatialResection::resectAll, py::arg("cameras"), py::arg("fromCurrentValues") = false,
                      py::arg("sigma2apriori") = 1.0, py::arg("rejectThreshold") = 0.0, py::arg("minPoints") = 4)
        .def_static("getMaximalNumberOfIterations", &SpatialResection::getMaximalNumberOfIterations)
        .def_static("setMaximalNumberOfIterations", &SpatialResection::setMaximalNumberOfIterations);
    py::class_<RelativeOrientation> relor(m, "RelativeOrientation");
    py::class_<RelativeOrientation::Result>(relor, "Result")
        .def_property_readonly("a", [](RelativeOrientation::Result &r) { return r.a; }, py::return_value_policy::reference)
        .def_property_readonly("b", [](RelativeOrientation::Result &r) { return r.b; }, py::return_value_policy::reference)
        .def_readonly("status", &RelativeOrientation::Result::status)
        .def_readonly("iterations", &RelativeOrientation::Result::iterations)
        .def_readonly("startKind", &RelativeOrientation::Result::startKind)
        .def_readonly("points", &RelativeOrientation::Result::points)
        .def_readonly("pointsUsed", &RelativeOrientation::Result::pointsUsed)
        .def("values", [](RelativeOrientation::Result &r) { return std::vector<double>(r.values, r.values + JAICOV_RELOR_OUT_PER_PAIR); });
    relor.def_static("orientAll", &RelativeOrientation::orientAll, py::arg("pairs"), py::arg("fromCurrentValues") = false,
                     py::arg("sigma2apriori") = 1.0, py::arg("rejectThreshold") = 0.0, py::arg("minPoints") = 6)
        .def_static("apply", &RelativeOrientation::apply, py::arg("result"), py::arg("baseLength") = 1.0)
        .def_static("getMaximalNumberOfIterations", &RelativeOrientation::getMaximalNumberOfIterations)
        .def_static("setMaximalNumberOfIterations", &RelativeOrientation::setMaximalNumberOfIterations);

    py::class_<SimilarityTransformation> simil(m, "SimilarityTransformation");
    py::class_<SimilarityTransformation::Model>(simil, "Model")
        .def(py::init<>())
        .def_readwrite("points", &SimilarityTransformation::Model::points)
        .def_readwrite("target", &SimilarityTransformation::Model::target)
        .def_readwrite("cofSource", &SimilarityTransformation::Model::cofSource)
        .def_readwrite("cofTarget", &SimilarityTransformation::Model::cofTarget);
    py::class_<SimilarityTransformation::Result>(simil, "Result")
        .def_readonly("status", &SimilarityTransformation::Result::status)
        .def_readonly("iterations", &SimilarityTransformation::Result::iterations)
        .def_readonly("startKind", &SimilarityTransformation::Result::startKind)
        .def_readonly("points", &SimilarityTransformation::Result::points)
        .def_readonly("pointsUsed", &SimilarityTransformation::Result::pointsUsed)
        .def_readonly("used", &SimilarityTransformation::Result::used)
        .def_readonly("q", &SimilarityTransformation::Result::q)
        .def("values", [](SimilarityTransformation::Result &r) { return std::vector<double>(r.values, r.values + JAICOV_SIMIL_OUT_PER_MODEL); });
    simil.def_static("estimateAll", &SimilarityTransformation::estimateAll, py::arg("models"), py::arg("rejectThreshold") = 0.0,
                     py::arg("minPoints") = 3)
        .def_static("apply", &SimilarityTransformation::apply, py::arg("result"), py::arg("points"), py::arg("images"))
        .def_static("getMaximalNumberOfIterations", &SimilarityTransformation::getMaximalNumberOfIterations)
        .def_static("setMaximalNumberOfIterations", &SimilarityTransformation::setMaximalNumberOfIterations);

    py::class_<LensCorrection> lens(m, "LensCorrection");
    py::class_<LensCorrection::Result>(lens, "Result")
        .def(py::init<>())
        .def_property("coordinate", [](LensCorrection::Result &r) { return r.coordinate; },
                      [](LensCorrection::Result &r, ImageCoordinate *ic) { r.coordinate = ic; }, py::return_value_policy::reference)
        .def_readwrite("x", &LensCorrection::Result::x)
        .def_readwrite("y", &LensCorrection::Result::y)
        .def_readwrite("varianceX", &LensCorrection::Result::varianceX)
        .def_readwrite("varianceY", &LensCorrection::Result::varianceY)
        .def_readwrite("rho", &LensCorrection::Result::rho)
        .def_readwrite("status", &LensCorrection::Result::status)
        .def_readwrite("iterations", &LensCorrection::Result::iterations);
    py::class_<LensCorrection::Scope>(lens, "Scope")
        .def(py::init<const std::vector<LensCorrection::Result> &>(), py::arg("results"))
        .def("applied", &LensCorrection::Scope::applied);
    lens.def_static("correctAll", &LensCorrection::correctAll, py::arg("camera"), py::arg("withDistance") = false, py::arg("tolerance") = 0.0)
        .def_static("distortAll", &LensCorrection::distortAll, py::arg("camera"), py::arg("withDistance") = false)
        .def_static("getMaximalNumberOfIterations", &LensCorrection::getMaximalNumberOfIterations)
        .def_static("setMaximalNumberOfIterations", &LensCorrection::setMaximalNumberOfIterations);

    py::class_<AiconProject>(m, "AiconProject")
        .def_property_readonly("camera", [](AiconProject &p) { return p.camera ? p.camera.get() : (p.cameras.empty() ? nullptr : p.cameras[0].get()); },
                               py::return_value_policy::reference_internal)
        .def("cameras", [](AiconProject &p) {
            std::vector<Camera *> v;
            if (p.camera) v.push_back(p.camera.get());
            for (auto &q : p.cameras) v.push_back(q.get());
            return v;
        }, py::return_value_policy::reference_internal)
        .def("points", [](AiconProject &p) {
            std::vector<ObjectCoordinate *> v;
            for (auto &q : p.points) v.push_back(q.get());
            return v;
        }, py::return_value_policy::reference_internal)
        .def("point", [](AiconProject &p, const std::string &n) { return p.byName.at(n); }, py::return_value_policy::reference_internal)
        .def("scaleBars", [](AiconProject &p) {
            std::vector<ScaleBar *> v;
            for (auto &q : p.scaleBars) v.push_back(q.get());
            return v;
        }, py::return_value_policy::reference_internal);
    m.def("read_aicon_flat", [](const std::string &base, std::vector<DistortionModel::Type> extra) { return read_aicon_flat(base, extra).release(); },
          py::arg("base"), py::arg("extra") = std::vector<DistortionModel::Type>{}, py::return_value_policy::take_ownership,
          "AICON flat files <base>.{obc,ior,scale,eor,phc} -> object graph (ExampleFlatFiles.java:76-103)");
    m.def("read_aicon_report", [](const std::string &path) { return read_aicon_report(path).release(); }, py::return_value_policy::take_ownership,
          "AICON 3D Studio adjustment report (.htm) -> object graph (AICONReportFileReader.java:117-390)");
}
