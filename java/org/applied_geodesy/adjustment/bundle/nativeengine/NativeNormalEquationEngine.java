/*
 * Reference-side binding (not compiled in this repository: the build image has no JDK; tests/test_jni_binding.py checks it
 * against the JNI shim and the C header at the text level).
 * A JAICOV maintainer adds this class next to org.applied_geodesy.adjustment.bundle.BundleAdjustment and replaces the
 * three call sites named in INTEGRATION.md.  It flattens the object graph once (after prepareUnknownParameters) and
 * forwards the per-iteration calls to libjaicov_neq.so through the JNI shim java/jni/jaicov_jni.c.
 */
package org.applied_geodesy.adjustment.bundle.nativeengine;

public final class NativeNormalEquationEngine implements AutoCloseable {
	static { System.loadLibrary("jaicov_jni"); }      // which in turn links libjaicov_neq.so

	private long handle;                                // jaicov_engine*

	/** Mirrors jaicov_problem_desc (include/jaicov_neq.h); every array is what BA:667-782 produced. */
	public static final class ProblemDescription {
		public int numberOfUnknowns, rankDefect, datumFlags;
		public int[] pointColumn, interiorColumn, cameraDistortionBegin, distortionKind, distortionOrder, distortionColumn;
		public int[] imageCamera, exteriorColumn, imagePointImage, imagePointPoint, blockBegin, scaleBarA, scaleBarB;
		public int[] directRowBegin, directSlot;
		public byte[] pointDatum;
		public double[] cameraR0, x, y, varianceX, varianceY, rho, blockDispersion, scaleBarLength, scaleBarVariance;
		public double[] directObservation, directVariance, directDispersion;
		public long[] blockDispersionOffset, directDispersionOffset;
	}

	/**
	 * Mirrors jaicov_engine_options (include/jaicov_neq.h), field for field; 0 = the engine's default everywhere.  This is the
	 * configuration surface next to the reference's setters (BundleAdjustment.java:1123-1195): what those cannot express because the
	 * pure-Java loop has no such choice (summation order, refinement of the step, which groups are pre-eliminated, the sharding).
	 */
	public static final class EngineOptions {
		public int device = 0;
		/** this engine accumulates the images [imageBegin, imageEnd) only; -1 / -1 = all images */
		public int imageBegin = -1, imageEnd = -1;
		/** the rank that adds scale bars, directly observed groups, datum, damping (rank 0 of a sharded run) */
		public boolean applyShared = true;
		/** 0 structure-aware (product), 1 dense J'WJ contraction on the matrix cores, 2 the same with fp32 accumulation (measuring mode) */
		public int assemblyMode = 0;
		public int blockSize = 0;
		/** != 0: MatrixInversion.REDUCED's last pass leaves in the EO entries of dx what BA:261-273 leaves there (SURVEY quirk Q1) */
		public int reducedReferenceQuirk = 0;
		/** 0 = default = fixed summation order (bit-reproducible, like the reference); < 0 = arrival-order sums (0.3 ms per pass faster at config 4) */
		public int deterministic = 0;
		/** steps of iterative refinement per solve: 0 = default (one), < 0 none, at most 4 */
		public int refinement = 0;
		/** < 0: ordinary ImageCoordinate groups stay outside the EO pre-elimination (rounds 1-3 path) */
		public int ordinaryGroupElimination = 0;
		/** < 0: inverse dispersions as the blocked Cholesky leaves them (no Newton-Schulz step) */
		public int dispersionRefinement = 0;
		/** != 0 on a sharded engine: the host sums expansionBuffer() over the ranks before an inverting solve with invert = 3 */
		public int expansionExchange = 0;
		/** < 0: no Newton-Schulz step on the inverse of systems of order <= 8192 (the step takes Qxx from 3e-9 to 1e-12 of the exact inverse at config 3) */
		public int inverseRefinement = 0;

		/** the options BundleAdjustment.native.patch reads from system properties, next to org.applied_geodesy.adjustment.bundle.native */
		public static EngineOptions fromSystemProperties() {
			EngineOptions o = new EngineOptions();
			o.device = Integer.getInteger("org.applied_geodesy.adjustment.bundle.native.device", 0);
			o.reducedReferenceQuirk = Boolean.getBoolean("org.applied_geodesy.adjustment.bundle.native.reducedReferenceQuirk") ? 1 : 0;
			o.deterministic = Integer.getInteger("org.applied_geodesy.adjustment.bundle.native.deterministic", 0);
			o.refinement = Integer.getInteger("org.applied_geodesy.adjustment.bundle.native.refinement", 0);
			return o;
		}
	}

	/** all images on one device */
	public NativeNormalEquationEngine(ProblemDescription d, int device) { this(d, device, -1, -1, true); }
	/** one rank of a sharded run: images [imageBegin, imageEnd); applyShared on the rank that adds scale bars and directly observed groups */
	public NativeNormalEquationEngine(ProblemDescription d, int device, int imageBegin, int imageEnd, boolean applyShared) {
		this(d, shard(device, imageBegin, imageEnd, applyShared));
	}
	/** every option of jaicov_engine_options */
	public NativeNormalEquationEngine(ProblemDescription d, EngineOptions options) {
		this.handle = create(d, options);                    // throws on failure (status mapped as in check())
	}
	private static EngineOptions shard(int device, int imageBegin, int imageEnd, boolean applyShared) {
		EngineOptions o = new EngineOptions();
		o.device = device; o.imageBegin = imageBegin; o.imageEnd = imageEnd; o.applyShared = applyShared;
		return o;
	}
	/** JAICOV_NEQ_ABI_VERSION of the loaded library */
	public static int abiVersion() { return abiVersion0(); }

	/** BA:235 createNormalEquation() */
	public void build(double sigma2apriori, double lambda, boolean simulation) { check(build(handle, sigma2apriori, lambda, simulation)); }
	/** multi-GPU form of build(): accumulate() -> all-reduce of reduceBuffer() over the ranks -> finish() */
	public void accumulate(double sigma2apriori, double lambda) { check(accumulate(handle, sigma2apriori, lambda)); }
	public void finish(double sigma2apriori, double lambda, boolean simulation) { check(finish(handle, sigma2apriori, lambda, simulation)); }
	/** {device address, count of doubles} of this rank's packed partial normal equations (ncclAllReduce, sum, double) */
	public long[] reduceBuffer() { long[] r = new long[2]; check(reduceBuffer(handle, r)); return r; }
	/**
	 * The same buffer without a host wait: {device address, count, hipStream_t}.  The buffer is complete in the order of that stream: enqueue
	 * the collective on it (ncclAllReduce(..., stream)) and finish() waits for it on the device -- the host never blocks between assembly and solve.
	 */
	public long[] reduceBufferAsync() { long[] r = new long[3]; check(reduceBufferAsync(handle, r)); return r; }
	/**
	 * {device address, count} of [F | L_E^-1] for the FINAL pass of MatrixInversion.FULL on a sharded engine (BA:268-271 per rank): this
	 * rank's images filled, zeros elsewhere.  Sum over the ranks between the all-reduce of reduceBuffer() and finish(); then solve(3, dx).
	 * Needs EngineOptions.expansionExchange and prepareInverse(3) before accumulate().
	 */
	public long[] expansionBuffer() { long[] r = new long[2]; check(expansionBuffer(handle, r)); return r; }
	/**
	 * {device address, count} of the exterior-orientation steps this engine back-substituted in the last solve (6 per image, zeros for the
	 * other ranks' images): summed over the ranks they are the EO entries of dx (BA:273 leaves them in dx on an unsharded run).
	 */
	public long[] eoStepBuffer() { long[] r = new long[2]; check(eoStepBuffer(handle, r)); return r; }
	/** NES.applyPrecondition + MathExtension.solve(N, n, invert) + reverse preconditioning (BA:238,270-297) */
	public void solve(int invert, double[] dx) { check(solve(handle, invert, dx)); }
	/**
	 * MatrixInversion -> JAICOV_INVERT_*: NONE 0, FULL 1, REDUCED and PRE_ELIMINATION 2 (BA:65-70, 261-271).  3 = FULL_EXPANDED: the
	 * same matrix as FULL, expanded from the inverse of the EO-reduced system (faster and more accurate where the engine can
	 * pre-eliminate; served as FULL where it cannot) -- what the patched estimateModel() passes for MatrixInversion.FULL.
	 */
	public static int invertMode(Enum<?> matrixInversion) {
		switch (matrixInversion.name()) { case "NONE": return 0; case "FULL": return 1; default: return 2; }
	}
	/** announces the invert mode of the solve after the next build (BA:250: the final pass is known before it is built) */
	public void prepareInverse(int invert) { check(prepareInverse(handle, invert)); }
	/** order of the system the last build assembled: u + d, or numRows of BA:262 when the exterior orientations were pre-eliminated */
	public int reducedOrder() { return reducedOrder(handle); }
	/** order of the cofactor matrix of the last inverting solve: u + d (FULL) or numRows of BA:262 (REDUCED) */
	public int cofactorOrder() { return cofactorOrder(handle); }
	/** BA:472 getOmega(dx) */
	public double omega(double sigma2apriori, double[] dx) { double[] o = new double[1]; check(omega(handle, sigma2apriori, dx, o)); return o[0]; }
	/** BA:450 updateUnknownParameters(dx); returns max|dx| */
	public double update(double[] dx) { double[] m = new double[1]; check(update(handle, dx, m)); return m[0]; }
	public int numSlots() { return (int) numSlots(handle); }
	public long packedLength() { return packedLength(handle); }
	public void setParameters(double[] slots) { check(setParameters(handle, slots)); }
	public void getParameters(double[] slots) { check(getParameters(handle, slots)); }
	/** N (packed 'U', UpperSymmPackMatrix.getData() order) and n of the last build: BA:789 createNormalEquation()'s result */
	public void getNormal(double[] packedN, double[] n) { check(getNormal(handle, packedN, n)); }
	/** UpperSymmPackMatrix.getData() order (UPLO='U'), length order(order+1)/2 with order = cofactorOrder() */
	public void getCofactor(double[] packed) { check(getCofactor(handle, packed)); }
	/** Qxx[indices, indices] as a dense row-major k x k block gathered on the device (MatlabResultWriter.java:210-221) */
	public double[] getCofactorSub(int[] indices) {
		double[] out = new double[indices.length * indices.length];
		check(getCofactorSub(handle, indices, out));
		return out;
	}
	/**
	 * scale * Qxx[indices, indices] as a dense row-major k x k block, gathered (and scaled) on the device: what
	 * DefaultResultWriter.java:139-147 (scale = sigma2apost) reads element by element from the packed matrix.
	 */
	public double[] getDispersionSub(double scale, int[] indices) {
		double[] out = new double[indices.length * indices.length];
		check(getDispersionSub(handle, scale, indices, out));
		return out;
	}
	/**
	 * BA.estimateModel() (BA:203-387) run natively: {state (EstimationStateType id), iterations, omega, max|dx|, final lambda,
	 * seconds total, seconds of the last pass}.  interrupt() from another thread ends it with state -1 (BA:240, 320).
	 */
	public double[] estimate(int maxIterations, int invert, boolean simulation, double lambda0, double sigma2apriori) {
		double[] r = new double[7];
		check(estimate(handle, maxIterations, invert, simulation, lambda0, sigma2apriori, r));
		return r;
	}
	/** BundleAdjustment.interrupt() (BA:1455) */
	public void interrupt() { check(cancel(handle)); }
	/** stage times of the last pass, ms: rows, assembly, finalize, factor, solve, inverse, omega, total (jaicov_neq_last_timings) */
	public double[] lastTimings() { double[] t = new double[8]; check(lastTimings(handle, t)); return t; }
	/** stage times of the engine's creation, ms (jaicov_neq_create_timings) */
	public double[] createTimings() { double[] t = new double[8]; check(createTimings(handle, t)); return t; }
	/** per-launch HIP events around the factorisation kernel on / off (jaicov_neq_set_profiling) */
	public void setProfiling(boolean on) { check(setProfiling(handle, on)); }
	/** counters of the engine (jaicov_neq_kernel_stats): factorisation launches, ms, flops, ..., abandoned factorisations [6], ... */
	public double[] kernelStats(boolean reset) { double[] s = new double[16]; check(kernelStats(handle, s, reset)); return s; }
	/** misclosures w (2 per image point) and Jacobian rows A (2 x (12 + distortion parameters) per image point) of [begin, begin + count): PDF:285-445 */
	public void getRows(int begin, int count, double[] w, double[] A) { check(getRows(handle, begin, count, w, A)); }
	/** the weight matrix sigma0^2-free inv(D) of jointly dispersed image block `block`, row-major m x m (DOPG:82-86 getWeightMatrix) */
	public void getBlockWeight(int block, double[] out) { check(getBlockWeight(handle, block, out)); }

	/**
	 * CoordinateTransformationExteriorOrientation.transform (tranformation/CoordinateTransformationExteriorOrientation.java:49-121) on
	 * the device, after an inverting solve that left all of Qxx (JAICOV_INVERT_FULL / _FULL_EXPANDED): points = the engine indices of
	 * the Set in iteration order, pairRef[k] / pairSrc[k] = the Map<Image, ArrayList<Image>> flattened in iteration order.  Returns the
	 * number of transformed points n (3 n rows); the covariance sigma2 J Qxx J' stays on the device (include/jaicov_transform.h).
	 */
	public int transform(int[] points, int[] pairRef, int[] pairSrc, double sigma2) {
		if (pairRef.length != pairSrc.length) throw new IllegalArgumentException("pairRef and pairSrc differ in length");
		long[] n = new long[1];
		check(xformRun(handle, points, pairRef, pairSrc, sigma2, n));
		return (int) n[0];
	}
	/** X, Y, Z of the n transformed points (xyz: 3 n) and their (point, src image, ref image) indices (ids: 3 n) */
	public void getTransformedCoordinates(double[] xyz, long[] ids) { check(xformGetCoordinates(handle, xyz, ids)); }
	/** the whole covariance, packed 'U' (UpperSymmPackMatrix.getData()) of order R = 3 n: refused when R (R + 1) / 2 exceeds a Java array */
	public double[] getTransformedCovariance(int n) {
		long R = 3L * n, len = R * (R + 1) / 2;
		if (len > Integer.MAX_VALUE - 8) throw new IllegalArgumentException("covariance of order " + R + " exceeds a Java array: use getTransformedCovarianceSub");
		double[] out = new double[(int) len];
		check(xformGetCovariance(handle, out));
		return out;
	}
	/** C[rows, rows] as a dense row-major k x k block gathered on the device (e.g. the 3 x 3 diagonal block of one point) */
	public double[] getTransformedCovarianceSub(int[] rows) {
		double[] out = new double[rows.length * rows.length];
		check(xformGetCovarianceSub(handle, rows, out));
		return out;
	}
	/** every 3 x 3 diagonal block (the covariance of each transformed point), 9 n doubles, row-major per block */
	public double[] getTransformedPointBlocks(int n) {
		double[] out = new double[9 * n];
		check(xformGetPointBlocks(handle, out));
		return out;
	}
	/** frees the device result of transform() */
	public void releaseTransformation() { check(xformRelease(handle)); }

	/**
	 * Residuals v = A dx - w, residual cofactors qvv, redundancy numbers r and test values t of every observation row, in the order of
	 * BundleAdjustment.java:670-771, after an inverting solve that left all of Qxx (JAICOV_INVERT_FULL / _FULL_EXPANDED).  sigma2Test:
	 * the a-priori variance factor (Baarda's w-test) or the a-posteriori one (Pope's tau); dx: null (a zero step) or the step of the
	 * inverting solve before update (exactly U doubles).  Returns the number of rows; the result stays on the device
	 * (include/jaicov_reliability.h).
	 */
	public int reliability(double sigma2Test, double[] dx) {
		long[] n = new long[1];
		check(relRun(handle, sigma2Test, dx, n));
		return (int) n[0];
	}
	/** the four vectors of the last reliability() (any array may be null, else n long; t is NaN for an uncontrolled row) */
	public void getReliability(int n, double[] v, double[] qvv, double[] r, double[] t) { check(relGet(handle, n, v, qvv, r, t)); }
	/** [0] sum of r, [1] max |t|, [2] its row, [3] rows with NaN t, [4] min r, [5] the damping of the inverted build (sum r = f needs 0) */
	public double[] getReliabilitySummary() {
		double[] out = new double[6];
		check(relSummary(handle, out));
		return out;
	}
	/** frees the device result of reliability() */
	public void releaseReliability() { check(relRelease(handle)); }

	/**
	 * Re-expresses the cofactor matrix of the last inverting solve, in place on the device, in the datum of the object points with
	 * pointDatum[i] != 0 (one entry per point, the meaning of the problem's point_datum; Baarda's S-transformation,
	 * include/jaicov_datum.h).  Needs a free network (d > 0); getCofactor, getCofactorSub, getDispersionSub, the writers and
	 * transform() see the new datum until the next inverting solve.
	 */
	public void transformDatum(int[] pointDatum) { check(datumTransform(handle, pointDatum)); }
	/** S v with the S of the last transformDatum (v.length >= cofactorOrder()): brings a coordinate difference into that datum */
	public double[] applyDatumTransformation(double[] v) {
		final int n = cofactorOrder(handle);
		double[] out = new double[Math.max(n, 0)];
		check(datumApply(handle, v, out, n));
		return out;
	}

	/** jaicov_dlt status values (include/jaicov_dlt.h) */
	public static final int DLT_CONVERGED = 0, DLT_NOT_CONVERGED = 1, DLT_TOO_FEW_POINTS = 2, DLT_SINGULAR = 3, DLT_NOT_FINITE = 4;

	/**
	 * DirectLinearTransformation.adjust (dlt/DirectLinearTransformation.java:67-169) for every image at once, on the device, with no
	 * engine: obsBegin (n + 1 CSR offsets) selects each image's homologous points, in the image's order (DT:73-94); xy = 2 doubles and
	 * xyz = 3 doubles per point (the control map's X, Y, Z); io = x0, y0, c per image; ioFixed (may be null) = 1 for a FIXED x0 / y0 / c;
	 * restrictions = RestrictionType ordinals in the caller's order (duplicates are dropped as DT:269-278 drops them).  out receives the
	 * 20 DLTCoefficients values per image (b11..b33, x0, y0, c, X0, Y0, Z0, omega, phi, kappa); the result is the status per image
	 * (DLT_CONVERGED is adjust()'s true).  Quirks Q1-Q3 of include/jaicov_dlt.h apply: for a camera with c < 0 the start value of
	 * kappa is out[19] + pi.
	 */
	public static long[] adjustDLT(int[] obsBegin, double[] xy, double[] xyz, double[] io, int[] ioFixed, int[] restrictions,
	                               int maxIterations, double[] out) {
		int n = obsBegin.length - 1;
		long[] status = new long[Math.max(n, 0)], solves = new long[Math.max(n, 0)];
		int rc = dltAdjust(obsBegin, xy, xyz, io, ioFixed, restrictions, maxIterations, out, status, solves);
		if (rc == -1) throw new IllegalArgumentException("jaicov_dlt_adjust: bad argument");
		if (rc == -4) throw new OutOfMemoryError("jaicov_dlt_adjust");
		if (rc != 0) throw new IllegalStateException("jaicov_dlt_adjust failed with status " + rc);
		return status;
	}

	/** jaicov_isect status values (include/jaicov_intersect.h) */
	public static final int ISECT_OK = 0, ISECT_NOT_CONVERGED = 1, ISECT_TOO_FEW_RAYS = 2, ISECT_SINGULAR = 3, ISECT_NOT_FINITE = 4;

	/**
	 * Spatial forward intersection of every object point of a batch from the image rays that see it, on the device, with no engine
	 * (include/jaicov_intersect.h; the reference has no counterpart: it reads the points' start values from a file).  rayBegin (n + 1
	 * CSR offsets) selects each point's rays; rayImage = the image of each ray; xy = 2 doubles per ray; var (may be null: unit
	 * weights) = variance x, variance y, correlation coefficient per ray (PartialDerivativeFactory.java:308-319); imageIo = x0, y0, c
	 * and imageEo = X0, Y0, Z0, omega, phi, kappa per image.  out receives 11 values per point (X, Y, Z, the six cofactors, Omega, the
	 * largest angle between two rays); iterations, rayUsed and rayQ may be null.  The result is the status per point; a point whose
	 * status is ISECT_TOO_FEW_RAYS, ISECT_SINGULAR or ISECT_NOT_FINITE has NaN values.
	 */
	public static long[] intersectPoints(int[] rayBegin, int[] rayImage, double[] xy, double[] var, double[] imageIo, double[] imageEo,
	                                     double sigma2apriori, int maxIterations, double rejectThreshold, int minRays, double[] out,
	                                     long[] iterations, long[] rayUsed, double[] rayQ) {
		int n = rayBegin.length - 1;
		long[] status = new long[Math.max(n, 0)];
		int rc = isectPoints(rayBegin, rayImage, xy, var, imageIo.length / 3, imageIo, imageEo, sigma2apriori, maxIterations, rejectThreshold,
		                     minRays, out, status, iterations, rayUsed, rayQ);
		if (rc == -1) throw new IllegalArgumentException("jaicov_isect_points: bad argument");
		if (rc == -4) throw new OutOfMemoryError("jaicov_isect_points");
		if (rc != 0) throw new IllegalStateException("jaicov_isect_points failed with status " + rc);
		return status;
	}

	/** jaicov_resect status values and start kinds (include/jaicov_resect.h) */
	public static final int RESECT_OK = 0, RESECT_NOT_CONVERGED = 1, RESECT_TOO_FEW_POINTS = 2, RESECT_SINGULAR = 3, RESECT_NOT_FINITE = 4;
	public static final int RESECT_START_GIVEN = 0, RESECT_START_SPACE = 1, RESECT_START_PLANE = 2;

	/**
	 * Spatial resection of every image of a batch from the known object points it sees and its known interior orientation, on the
	 * device, with no engine (include/jaicov_resect.h; the reference has no counterpart).  obsBegin (n + 1 CSR offsets) selects each
	 * image's observations; xy = 2 doubles and xyz = 3 doubles (the object point) per observation; var (may be null: unit weights) =
	 * variance x, variance y, correlation coefficient per observation (PartialDerivativeFactory.java:308-319); imageIo = x0, y0, c per
	 * image, c of either sign; eoStart (may be null) = X0, Y0, Z0, omega, phi, kappa per image: an image whose six values are finite
	 * starts from them, any other from the linear start.  out receives 28 values per image (X0, Y0, Z0, omega, phi, kappa, the upper
	 * triangle of the cofactor matrix, Omega); iterations, startKind, obsUsed and obsQ may be null.  The result is the status per image;
	 * an image whose status is RESECT_TOO_FEW_POINTS, RESECT_SINGULAR or RESECT_NOT_FINITE has NaN values.
	 */
	public static long[] resectImages(int[] obsBegin, double[] xy, double[] xyz, double[] var, double[] imageIo, double[] eoStart,
	                                  double sigma2apriori, int maxIterations, double rejectThreshold, int minPoints, double[] out,
	                                  long[] iterations, long[] startKind, long[] obsUsed, double[] obsQ) {
		int n = obsBegin.length - 1;
		long[] status = new long[Math.max(n, 0)];
		int rc = resectImages(obsBegin, xy, xyz, var, imageIo, eoStart, sigma2apriori, maxIterations, rejectThreshold, minPoints, out, status,
		                      iterations, startKind, obsUsed, obsQ);
		if (rc == -1) throw new IllegalArgumentException("jaicov_resect_images: bad argument");
		if (rc == -4) throw new OutOfMemoryError("jaicov_resect_images");
		if (rc != 0) throw new IllegalStateException("jaicov_resect_images failed with status " + rc);
		return status;
	}

	/** jaicov_relorient status values and start kinds (include/jaicov_relorient.h) */
	public static final int RELOR_OK = 0, RELOR_NOT_CONVERGED = 1, RELOR_TOO_FEW_POINTS = 2, RELOR_SINGULAR = 3, RELOR_NOT_FINITE = 4;
	public static final int RELOR_START_GIVEN = 0, RELOR_START_SPACE = 1, RELOR_START_PLANE = 2;

	/**
	 * Relative orientation of every image pair of a batch from the image points the two images share and their known interior
	 * orientations, on the device, with no engine (include/jaicov_relorient.h; the reference has no counterpart).  obsBegin (n + 1 CSR
	 * offsets) selects each pair's observations; xyA and xyB = 2 doubles per observation, the same object point in image a and in image
	 * b; varA, varB (either may be null) = variance x, variance y, correlation coefficient per observation
	 * (PartialDerivativeFactory.java:308-319); pairIo = x0, y0, c of image a's camera, then of image b's, per pair, c of either sign;
	 * start (may be null) = X0, Y0, Z0, omega, phi, kappa of image b in the frame of image a per pair: a pair whose six values are
	 * finite starts from them, any other from the linear starts.  out receives 28 values per pair (X0, Y0, Z0 of unit length, omega, phi,
	 * kappa, the upper triangle of the cofactor matrix, Omega); iterations, startKind, obsUsed and obsQ may be null.  The result is the
	 * status per pair; a pair whose status is RELOR_TOO_FEW_POINTS, RELOR_SINGULAR or RELOR_NOT_FINITE has NaN values.
	 */
	public static long[] orientPairs(int[] obsBegin, double[] xyA, double[] xyB, double[] varA, double[] varB, double[] pairIo, double[] start,
	                                 double sigma2apriori, int maxIterations, double rejectThreshold, int minPoints, double[] out,
	                                 long[] iterations, long[] startKind, long[] obsUsed, double[] obsQ) {
		int n = obsBegin.length - 1;
		long[] status = new long[Math.max(n, 0)];
		int rc = orientPairs(obsBegin, xyA, xyB, varA, varB, pairIo, start, sigma2apriori, maxIterations, rejectThreshold, minPoints, out, status,
		                     iterations, startKind, obsUsed, obsQ);
		if (rc == -1) throw new IllegalArgumentException("jaicov_relorient_pairs: bad argument");
		if (rc == -4) throw new OutOfMemoryError("jaicov_relorient_pairs");
		if (rc != 0) throw new IllegalStateException("jaicov_relorient_pairs failed with status " + rc);
		return status;
	}

	/** jaicov_simil status values and start kinds (include/jaicov_simil.h) */
	public static final int SIMIL_OK = 0, SIMIL_NOT_CONVERGED = 1, SIMIL_TOO_FEW_POINTS = 2, SIMIL_SINGULAR = 3, SIMIL_NOT_FINITE = 4;
	public static final int SIMIL_START_GIVEN = 0, SIMIL_START_CLOSED = 1;

	/**
	 * Absolute orientation of every model of a batch: the spatial similarity transformation dst = T + m R src between two sets of the
	 * same points, on the device, with no engine (include/jaicov_simil.h; the reference has no counterpart).  ptBegin (n + 1 CSR
	 * offsets) selects each model's points; src and dst = 3 doubles per point, the point in the model's frame and in the target frame;
	 * cofSrc, cofDst (either may be null: 0 and I) = qXX qXY qXZ qYY qYZ qZZ per point; start (may be null) = Tx, Ty, Tz, m, omega, phi,
	 * kappa per model: a model whose seven values are finite starts from them, any other from the closed start.  out receives 36
	 * values per model (Tx, Ty, Tz, m, omega, phi, kappa, the upper triangle of their cofactor matrix, Omega); iterations, startKind,
	 * ptUsed and ptQ may be null.  The result is the status per model; a model whose status is SIMIL_TOO_FEW_POINTS, SIMIL_SINGULAR or
	 * SIMIL_NOT_FINITE has NaN values.
	 */
	public static long[] similarityModels(int[] ptBegin, double[] src, double[] dst, double[] cofSrc, double[] cofDst, double[] start,
	                                      int maxIterations, double rejectThreshold, int minPoints, double[] out, long[] iterations,
	                                      long[] startKind, long[] ptUsed, double[] ptQ) {
		int n = ptBegin.length - 1;
		long[] status = new long[Math.max(n, 0)];
		int rc = similModels(ptBegin, src, dst, cofSrc, cofDst, start, maxIterations, rejectThreshold, minPoints, out, status, iterations,
		                     startKind, ptUsed, ptQ);
		if (rc == -1) throw new IllegalArgumentException("jaicov_simil_models: bad argument");
		if (rc == -4) throw new OutOfMemoryError("jaicov_simil_models");
		if (rc != 0) throw new IllegalStateException("jaicov_simil_models failed with status " + rc);
		return status;
	}

	/**
	 * Carries the points and the image orientations of every model into the target frame (include/jaicov_simil.h).  par = 7 doubles
	 * per model, the first seven values of similarityModels' out; ptBegin (may be null: no points) with xyz (3 per point), cof (6 per
	 * point, may be null) and their outputs xyzOut, cofOut; imgBegin (may be null: no orientations) with eo (X0, Y0, Z0, omega, phi,
	 * kappa per image) and eoOut.  The dispersion of the seven parameters is not propagated.
	 */
	public static void similarityApply(double[] par, int[] ptBegin, double[] xyz, double[] cof, int[] imgBegin, double[] eo, double[] xyzOut,
	                                   double[] cofOut, double[] eoOut) {
		int rc = similApply(par, ptBegin, xyz, cof, imgBegin, eo, xyzOut, cofOut, eoOut);
		if (rc == -1) throw new IllegalArgumentException("jaicov_simil_apply: bad argument");
		if (rc == -4) throw new OutOfMemoryError("jaicov_simil_apply");
		if (rc != 0) throw new IllegalStateException("jaicov_simil_apply failed with status " + rc);
	}

	@Override public void close() { if (handle != 0) { destroy(handle); handle = 0; } }

	private void check(int status) {
		if (status == 0) return;
		String msg = lastError(handle);
		if (status > 0) throw new no.uib.cipr.matrix.MatrixSingularException();          // MX:350,361
		if (status == -4) throw new OutOfMemoryError(msg);                                // BA:370-375
		if (status == -1) throw new IllegalArgumentException(msg);                        // MX:352,363
		throw new IllegalStateException(msg);
	}

	private static native long create(ProblemDescription d, EngineOptions options);
	private static native int abiVersion0();
	private static native int reduceBufferAsync(long h, long[] pointerCountStream);
	private static native int expansionBuffer(long h, long[] pointerAndCount);
	private static native int eoStepBuffer(long h, long[] pointerAndCount);
	private static native int lastTimings(long h, double[] ms);
	private static native int createTimings(long h, double[] ms);
	private static native int setProfiling(long h, boolean on);
	private static native int kernelStats(long h, double[] stats, boolean reset);
	private static native int getRows(long h, int begin, int count, double[] w, double[] A);
	private static native int getBlockWeight(long h, int block, double[] out);
	private static native void destroy(long h);
	private static native String lastError(long h);
	private static native long numSlots(long h);
	private static native long packedLength(long h);
	private static native int setParameters(long h, double[] slots);
	private static native int getParameters(long h, double[] slots);
	private static native int build(long h, double sigma2, double lambda, boolean simulation);
	private static native int accumulate(long h, double sigma2, double lambda);
	private static native int finish(long h, double sigma2, double lambda, boolean simulation);
	private static native int reduceBuffer(long h, long[] pointerAndCount);
	private static native int prepareInverse(long h, int invert);
	private static native int reducedOrder(long h);
	private static native int cofactorOrder(long h);
	private static native int solve(long h, int invert, double[] dx);
	private static native int omega(long h, double sigma2, double[] dx, double[] out);
	private static native int update(long h, double[] dx, double[] maxAbs);
	private static native int getNormal(long h, double[] packedN, double[] n);
	private static native int getCofactor(long h, double[] packed);
	private static native int getCofactorSub(long h, int[] indices, double[] out);
	private static native int getDispersionSub(long h, double scale, int[] indices, double[] out);
	private static native int estimate(long h, int maxIterations, int invert, boolean simulation, double lambda0, double sigma2apriori, double[] result);
	private static native int cancel(long h);
	private static native int xformRun(long h, int[] points, int[] pairRef, int[] pairSrc, double sigma2, long[] count);
	private static native int xformGetCoordinates(long h, double[] xyz, long[] ids);
	private static native int xformGetCovariance(long h, double[] packed);
	private static native int xformGetCovarianceSub(long h, int[] rows, double[] out);
	private static native int xformGetPointBlocks(long h, double[] out);
	private static native int xformRelease(long h);
	private static native int relRun(long h, double sigma2Test, double[] dx, long[] count);
	private static native int relGet(long h, int n, double[] v, double[] qvv, double[] r, double[] t);
	private static native int relSummary(long h, double[] out);
	private static native int relRelease(long h);
	private static native int datumTransform(long h, int[] pointDatum);
	private static native int datumApply(long h, double[] v, double[] out, int n);
	private static native int dltAdjust(int[] obsBegin, double[] xy, double[] xyz, double[] io, int[] ioFixed, int[] restrictions, int maxIterations, double[] out, long[] status, long[] solves);
	private static native int isectPoints(int[] rayBegin, int[] rayImage, double[] xy, double[] var, int nImages, double[] imageIo, double[] imageEo, double sigma2apriori, int maxIterations, double rejectThreshold, int minRays, double[] out, long[] status, long[] iterations, long[] rayUsed, double[] rayQ);
	private static native int resectImages(int[] obsBegin, double[] xy, double[] xyz, double[] var, double[] imageIo, double[] eoStart, double sigma2apriori, int maxIterations, double rejectThreshold, int minPoints, double[] out, long[] status, long[] iterations, long[] startKind, long[] obsUsed, double[] obsQ);
	private static native int orientPairs(int[] obsBegin, double[] xyA, double[] xyB, double[] varA, double[] varB, double[] pairIo, double[] start, double sigma2apriori, int maxIterations, double rejectThreshold, int minPoints, double[] out, long[] status, long[] iterations, long[] startKind, long[] obsUsed, double[] obsQ);
	private static native int similModels(int[] ptBegin, double[] src, double[] dst, double[] cofSrc, double[] cofDst, double[] start, int maxIterations, double rejectThreshold, int minPoints, double[] out, long[] status, long[] iterations, long[] startKind, long[] ptUsed, double[] ptQ);
	private static native int similApply(double[] par, int[] ptBegin, double[] xyz, double[] cof, int[] imgBegin, double[] eo, double[] xyzOut, double[] cofOut, double[] eoOut);
}
