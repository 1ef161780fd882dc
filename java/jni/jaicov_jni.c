/*
 * JNI shim between NativeNormalEquationEngine (Java) and the C ABI of include/jaicov_neq.h, include/jaicov_transform.h,
 * include/jaicov_dlt.h, include/jaicov_reliability.h, include/jaicov_datum.h, include/jaicov_intersect.h,
 * include/jaicov_resect.h, include/jaicov_relorient.h and include/jaicov_simil.h.
 * The build image has no JDK, so this file is not built by __graft_entry__.build(); on a box with a JDK:
 *   gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../../include jaicov_jni.c \
 *       -L../../bundle-adjustment_amd/csrc -ljaicov_neq -o libjaicov_jni.so
 * tests/test_jni_binding.py keeps it honest without one: every `native` method of the Java class has exactly one
 * Java_... function here (same arity), every jaicov_neq_* called here is declared in the header, and the file compiles
 * against a minimal jni.h (tests/jni_stub, test infrastructure only).
 *
 * Array policy.  create() COPIES the structure arrays (Get<Type>ArrayElements / Release with JNI_ABORT, one array at a
 * time, nothing held across jaicov_neq_create's device work except those copies).  The per-call double[] arguments are
 * pinned with GetPrimitiveArrayCritical for the duration of ONE jaicov_neq_* call; those calls make no JNI calls and the
 * engine is externally synchronised (one engine per BundleAdjustment), which is what the critical-region rules ask for.
 * Every pinned pointer is released with the pointer it was pinned with.
 */
#include <jni.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "jaicov_neq.h"
#include "jaicov_transform.h"
#include "jaicov_dlt.h"
#include "jaicov_intersect.h"
#include "jaicov_resect.h"
#include "jaicov_relorient.h"
#include "jaicov_simil.h"
#include "jaicov_reliability.h"
#include "jaicov_datum.h"

#define ENG(h) ((jaicov_engine *)(intptr_t)(h))
#define NAT(name) Java_org_applied_1geodesy_adjustment_bundle_nativeengine_NativeNormalEquationEngine_##name

static void throw_status(JNIEnv *e, int status, const char *msg) {
    const char *cls = status > 0 ? "no/uib/cipr/matrix/MatrixSingularException"          /* MX:350,361 */
                     : status == JAICOV_ERR_OUT_OF_MEMORY ? "java/lang/OutOfMemoryError"  /* BA:370-375 */
                     : status == JAICOV_ERR_BAD_ARGUMENT ? "java/lang/IllegalArgumentException" /* MX:352,363 */
                                                         : "java/lang/IllegalStateException";
    jclass c = (*e)->FindClass(e, cls);
    if (c) (*e)->ThrowNew(e, c, msg ? msg : "jaicov engine error");
}

/* one structure array of the problem description: a copy (or pin) obtained with the typed Get...Elements call */
typedef struct { jarray arr; void *ptr; char kind; jsize len; } held_t;

static int hold(JNIEnv *e, jobject obj, jclass c, const char *name, char kind, held_t *h) {
    char sig[3] = {'[', kind, 0};
    jfieldID f = (*e)->GetFieldID(e, c, name, sig);
    h->arr = NULL; h->ptr = NULL; h->kind = kind; h->len = 0;
    if (!f) return -1;                                   /* NoSuchFieldError is pending */
    h->arr = (jarray)(*e)->GetObjectField(e, obj, f);
    if (!h->arr) return 0;                               /* optional array absent */
    h->len = (*e)->GetArrayLength(e, h->arr);
    switch (kind) {
        case 'I': h->ptr = (*e)->GetIntArrayElements(e, (jintArray)h->arr, NULL); break;
        case 'J': h->ptr = (*e)->GetLongArrayElements(e, (jlongArray)h->arr, NULL); break;
        case 'B': h->ptr = (*e)->GetByteArrayElements(e, (jbyteArray)h->arr, NULL); break;
        default:  h->ptr = (*e)->GetDoubleArrayElements(e, (jdoubleArray)h->arr, NULL); break;
    }
    return h->ptr ? 0 : -1;                              /* OutOfMemoryError is pending */
}

static void unhold(JNIEnv *e, held_t *h) {
    if (!h->arr || !h->ptr) return;
    switch (h->kind) {
        case 'I': (*e)->ReleaseIntArrayElements(e, (jintArray)h->arr, (jint *)h->ptr, JNI_ABORT); break;
        case 'J': (*e)->ReleaseLongArrayElements(e, (jlongArray)h->arr, (jlong *)h->ptr, JNI_ABORT); break;
        case 'B': (*e)->ReleaseByteArrayElements(e, (jbyteArray)h->arr, (jbyte *)h->ptr, JNI_ABORT); break;
        default:  (*e)->ReleaseDoubleArrayElements(e, (jdoubleArray)h->arr, (jdouble *)h->ptr, JNI_ABORT); break;
    }
    h->ptr = NULL;
}

/* EngineOptions (Java) -> jaicov_engine_options, field for field; returns -1 with a JNI exception pending when a field is missing */
static int read_options(JNIEnv *e, jobject opt, jaicov_engine_options *o) {
    memset(o, 0, sizeof(*o));
    o->struct_size = sizeof(*o);
    o->image_begin = o->image_end = -1;
    o->apply_shared = 1;
    if (!opt) return 0;                                  /* null = all defaults, all images, device 0 */
    jclass oc = (*e)->GetObjectClass(e, opt);
    static const struct { const char *name; size_t off; } I[] = {
        {"device", offsetof(jaicov_engine_options, device)},
        {"imageBegin", offsetof(jaicov_engine_options, image_begin)},
        {"imageEnd", offsetof(jaicov_engine_options, image_end)},
        {"assemblyMode", offsetof(jaicov_engine_options, assembly_mode)},
        {"blockSize", offsetof(jaicov_engine_options, block_size)},
        {"reducedReferenceQuirk", offsetof(jaicov_engine_options, reduced_reference_quirk)},
        {"deterministic", offsetof(jaicov_engine_options, deterministic)},
        {"refinement", offsetof(jaicov_engine_options, refinement)},
        {"ordinaryGroupElimination", offsetof(jaicov_engine_options, ordinary_group_elimination)},
        {"dispersionRefinement", offsetof(jaicov_engine_options, dispersion_refinement)},
        {"expansionExchange", offsetof(jaicov_engine_options, expansion_exchange)},
        {"inverseRefinement", offsetof(jaicov_engine_options, inverse_refinement)}};
    for (size_t q = 0; q < sizeof(I) / sizeof(I[0]); q++) {
        jfieldID f = (*e)->GetFieldID(e, oc, I[q].name, "I");
        if (!f) return -1;
        *(int32_t *)((char *)o + I[q].off) = (int32_t)(*e)->GetIntField(e, opt, f);
    }
    jfieldID fs = (*e)->GetFieldID(e, oc, "applyShared", "Z");
    if (!fs) return -1;
    o->apply_shared = (*e)->GetBooleanField(e, opt, fs) ? 1 : 0;
    return 0;
}

JNIEXPORT jlong JNICALL NAT(create)(JNIEnv *e, jclass k, jobject d, jobject options) {
    (void)k;
    jaicov_engine_options o;
    if (read_options(e, options, &o)) return 0;
    jclass c = (*e)->GetObjectClass(e, d);
    jaicov_problem_desc p;
    memset(&p, 0, sizeof(p));
    p.struct_size = sizeof(p);
    jfieldID fu = (*e)->GetFieldID(e, c, "numberOfUnknowns", "I"), fr = (*e)->GetFieldID(e, c, "rankDefect", "I"),
             fd = (*e)->GetFieldID(e, c, "datumFlags", "I");
    if (!fu || !fr || !fd) return 0;
    p.n_unknowns = (*e)->GetIntField(e, d, fu);
    p.rank_defect = (*e)->GetIntField(e, d, fr);
    p.datum_flags = (*e)->GetIntField(e, d, fd);
    enum { POINT_COL, POINT_DATUM, IO_COL, CAM_R0, CAM_DIST_BEGIN, DIST_KIND, DIST_ORDER, DIST_COL, IMAGE_CAMERA, EO_COL, IP_IMAGE,
           IP_POINT, IP_X, IP_Y, IP_VX, IP_VY, IP_RHO, BLK_BEGIN, BLK_OFF, BLK_DISP, SB_A, SB_B, SB_LEN, SB_VAR, DG_BEGIN, DG_SLOT,
           DG_OBS, DG_VAR, DG_OFF, DG_DISP, N_HELD };
    static const struct { const char *name; char kind; } F[N_HELD] = {
        {"pointColumn", 'I'}, {"pointDatum", 'B'}, {"interiorColumn", 'I'}, {"cameraR0", 'D'}, {"cameraDistortionBegin", 'I'},
        {"distortionKind", 'I'}, {"distortionOrder", 'I'}, {"distortionColumn", 'I'}, {"imageCamera", 'I'}, {"exteriorColumn", 'I'},
        {"imagePointImage", 'I'}, {"imagePointPoint", 'I'}, {"x", 'D'}, {"y", 'D'}, {"varianceX", 'D'}, {"varianceY", 'D'}, {"rho", 'D'},
        {"blockBegin", 'I'}, {"blockDispersionOffset", 'J'}, {"blockDispersion", 'D'}, {"scaleBarA", 'I'}, {"scaleBarB", 'I'},
        {"scaleBarLength", 'D'}, {"scaleBarVariance", 'D'}, {"directRowBegin", 'I'}, {"directSlot", 'I'}, {"directObservation", 'D'},
        {"directVariance", 'D'}, {"directDispersionOffset", 'J'}, {"directDispersion", 'D'}};
    held_t a[N_HELD];
    int n = 0, bad = 0;
    for (; n < N_HELD && !bad; n++) bad = hold(e, d, c, F[n].name, F[n].kind, &a[n]);
    jaicov_engine *eng = NULL;
    int rc = JAICOV_ERR_BAD_ARGUMENT;
    char msg[512];
    msg[0] = 0;
    if (!bad) {
        p.point_col = (const int32_t *)a[POINT_COL].ptr;          p.point_datum = (const uint8_t *)a[POINT_DATUM].ptr;
        p.io_col = (const int32_t *)a[IO_COL].ptr;                p.cam_r0 = (const double *)a[CAM_R0].ptr;
        p.cam_dist_begin = (const int32_t *)a[CAM_DIST_BEGIN].ptr; p.dist_kind = (const int32_t *)a[DIST_KIND].ptr;
        p.dist_order = (const int32_t *)a[DIST_ORDER].ptr;        p.dist_col = (const int32_t *)a[DIST_COL].ptr;
        p.image_camera = (const int32_t *)a[IMAGE_CAMERA].ptr;    p.eo_col = (const int32_t *)a[EO_COL].ptr;
        p.ip_image = (const int32_t *)a[IP_IMAGE].ptr;            p.ip_point = (const int32_t *)a[IP_POINT].ptr;
        p.ip_x = (const double *)a[IP_X].ptr;                     p.ip_y = (const double *)a[IP_Y].ptr;
        p.ip_var_x = (const double *)a[IP_VX].ptr;                p.ip_var_y = (const double *)a[IP_VY].ptr;
        p.ip_rho = (const double *)a[IP_RHO].ptr;
        p.blk_ip_begin = (const int32_t *)a[BLK_BEGIN].ptr;       p.blk_disp_offset = (const int64_t *)a[BLK_OFF].ptr;
        p.blk_disp = (const double *)a[BLK_DISP].ptr;
        p.sb_point_a = (const int32_t *)a[SB_A].ptr;              p.sb_point_b = (const int32_t *)a[SB_B].ptr;
        p.sb_length = (const double *)a[SB_LEN].ptr;              p.sb_var = (const double *)a[SB_VAR].ptr;
        p.dg_row_begin = (const int32_t *)a[DG_BEGIN].ptr;        p.dg_slot = (const int32_t *)a[DG_SLOT].ptr;
        p.dg_obs = (const double *)a[DG_OBS].ptr;                 p.dg_var = (const double *)a[DG_VAR].ptr;
        p.dg_disp_offset = (const int64_t *)a[DG_OFF].ptr;        p.dg_disp = (const double *)a[DG_DISP].ptr;
        /* the n_* counts follow from the array lengths */
        p.n_points = a[POINT_COL].len / 3;
        p.n_cameras = a[IO_COL].len / 3;
        p.n_dist = a[DIST_KIND].len;
        p.n_images = a[IMAGE_CAMERA].len;
        p.n_image_points = a[IP_IMAGE].len;
        p.n_image_blocks = a[BLK_BEGIN].len > 0 ? a[BLK_BEGIN].len - 1 : 0;
        p.n_scale_bars = a[SB_A].len;
        p.n_direct_groups = a[DG_BEGIN].len > 0 ? a[DG_BEGIN].len - 1 : 0;
        p.n_direct_rows = a[DG_SLOT].len;
        rc = jaicov_neq_create(&p, &o, &eng);            /* copies everything it keeps */
        if (rc != JAICOV_OK) {
            strncpy(msg, eng ? jaicov_neq_last_error(eng) : "jaicov_neq_create failed", sizeof(msg) - 1);
            msg[sizeof(msg) - 1] = 0;
            jaicov_neq_destroy(eng);
            eng = NULL;
        }
    }
    while (n > 0) unhold(e, &a[--n]);
    if (bad) return 0;                                   /* the JNI exception of the failed lookup / copy is pending */
    if (rc != JAICOV_OK) { throw_status(e, rc, msg); return 0; }
    return (jlong)(intptr_t)eng;
}

JNIEXPORT void JNICALL NAT(destroy)(JNIEnv *e, jclass k, jlong h) { (void)e; (void)k; jaicov_neq_destroy(ENG(h)); }
JNIEXPORT jstring JNICALL NAT(lastError)(JNIEnv *e, jclass k, jlong h) { (void)k; return (*e)->NewStringUTF(e, jaicov_neq_last_error(ENG(h))); }
JNIEXPORT jlong JNICALL NAT(numSlots)(JNIEnv *e, jclass k, jlong h) { (void)e; (void)k; return (jlong)jaicov_neq_num_slots(ENG(h)); }
JNIEXPORT jlong JNICALL NAT(packedLength)(JNIEnv *e, jclass k, jlong h) { (void)e; (void)k; return (jlong)jaicov_neq_packed_length(ENG(h)); }

JNIEXPORT jint JNICALL NAT(setParameters)(JNIEnv *e, jclass k, jlong h, jdoubleArray s) {
    (void)k;
    jsize n = (*e)->GetArrayLength(e, s);
    double *p = (double *)(*e)->GetPrimitiveArrayCritical(e, s, NULL);
    if (!p) return JAICOV_ERR_OUT_OF_MEMORY;
    int rc = jaicov_neq_set_parameters(ENG(h), p, (size_t)n);
    (*e)->ReleasePrimitiveArrayCritical(e, s, p, JNI_ABORT);
    return rc;
}
JNIEXPORT jint JNICALL NAT(getParameters)(JNIEnv *e, jclass k, jlong h, jdoubleArray s) {
    (void)k;
    jsize n = (*e)->GetArrayLength(e, s);
    double *p = (double *)(*e)->GetPrimitiveArrayCritical(e, s, NULL);
    if (!p) return JAICOV_ERR_OUT_OF_MEMORY;
    int rc = jaicov_neq_get_parameters(ENG(h), p, (size_t)n);
    (*e)->ReleasePrimitiveArrayCritical(e, s, p, 0);
    return rc;
}
JNIEXPORT jint JNICALL NAT(build)(JNIEnv *e, jclass k, jlong h, jdouble s2, jdouble lambda, jboolean sim) {
    (void)e; (void)k;
    return jaicov_neq_build(ENG(h), s2, lambda, sim ? 1 : 0);
}
JNIEXPORT jint JNICALL NAT(accumulate)(JNIEnv *e, jclass k, jlong h, jdouble s2, jdouble lambda) {
    (void)e; (void)k;
    return jaicov_neq_accumulate2(ENG(h), s2, lambda);
}
JNIEXPORT jint JNICALL NAT(finish)(JNIEnv *e, jclass k, jlong h, jdouble s2, jdouble lambda, jboolean sim) {
    (void)e; (void)k;
    return jaicov_neq_finalize(ENG(h), s2, lambda, sim ? 1 : 0);
}
/* out[0] = DEVICE address of the packed partial normal equations, out[1] = number of doubles: what the host hands to
 * ncclAllReduce (sum, double) between accumulate() and finish() on a multi-GPU node */
JNIEXPORT jint JNICALL NAT(reduceBuffer)(JNIEnv *e, jclass k, jlong h, jlongArray out) {
    (void)k;
    void *ptr = NULL;
    size_t cnt = 0;
    int rc = jaicov_neq_reduce_buffer(ENG(h), &ptr, &cnt);
    jlong v[2] = {(jlong)(intptr_t)ptr, (jlong)cnt};
    if ((*e)->GetArrayLength(e, out) < 2) return JAICOV_ERR_BAD_ARGUMENT;
    (*e)->SetLongArrayRegion(e, out, 0, 2, v);
    return rc;
}
/* device pointer + count (+ stream) triples of the three exchange buffers of a sharded run */
static jint put_longs(JNIEnv *e, jlongArray out, int rc, const jlong *v, jsize n) {
    if ((*e)->GetArrayLength(e, out) < n) return JAICOV_ERR_BAD_ARGUMENT;
    (*e)->SetLongArrayRegion(e, out, 0, n, v);
    return rc;
}
/* out = {device address, count, hipStream_t}: the collective is enqueued on that stream, no host wait (jaicov_neq_reduce_buffer_async) */
JNIEXPORT jint JNICALL NAT(reduceBufferAsync)(JNIEnv *e, jclass k, jlong h, jlongArray out) {
    (void)k;
    void *ptr = NULL, *st = NULL;
    size_t cnt = 0;
    int rc = jaicov_neq_reduce_buffer_async(ENG(h), &ptr, &cnt, &st);
    jlong v[3] = {(jlong)(intptr_t)ptr, (jlong)cnt, (jlong)(intptr_t)st};
    return put_longs(e, out, rc, v, 3);
}
/* the sharded FINAL pass of MatrixInversion.FULL (BA:268-271 per rank): [F | L_E^-1] of this rank's images, summed over the ranks */
JNIEXPORT jint JNICALL NAT(expansionBuffer)(JNIEnv *e, jclass k, jlong h, jlongArray out) {
    (void)k;
    void *ptr = NULL;
    size_t cnt = 0;
    int rc = jaicov_neq_expansion_buffer(ENG(h), &ptr, &cnt);
    jlong v[2] = {(jlong)(intptr_t)ptr, (jlong)cnt};
    return put_longs(e, out, rc, v, 2);
}
/* the EO steps this rank back-substituted (6 per image), summed over the ranks into dx's EO entries */
JNIEXPORT jint JNICALL NAT(eoStepBuffer)(JNIEnv *e, jclass k, jlong h, jlongArray out) {
    (void)k;
    void *ptr = NULL;
    size_t cnt = 0;
    int rc = jaicov_neq_eo_step_buffer(ENG(h), &ptr, &cnt);
    jlong v[2] = {(jlong)(intptr_t)ptr, (jlong)cnt};
    return put_longs(e, out, rc, v, 2);
}
JNIEXPORT jint JNICALL NAT(abiVersion0)(JNIEnv *e, jclass k) { (void)e; (void)k; return jaicov_neq_abi_version(); }
/* small double[] out-parameters: filled through a stack copy (no array pinned across the call) */
static jint put_doubles(JNIEnv *e, jdoubleArray out, int rc, const double *v, jsize have) {
    jsize n = (*e)->GetArrayLength(e, out);
    (*e)->SetDoubleArrayRegion(e, out, 0, n < have ? n : have, v);
    return rc;
}
JNIEXPORT jint JNICALL NAT(lastTimings)(JNIEnv *e, jclass k, jlong h, jdoubleArray ms) {
    (void)k;
    double v[8] = {0};
    return put_doubles(e, ms, jaicov_neq_last_timings(ENG(h), v, 8), v, 8);
}
JNIEXPORT jint JNICALL NAT(createTimings)(JNIEnv *e, jclass k, jlong h, jdoubleArray ms) {
    (void)k;
    double v[8] = {0};
    return put_doubles(e, ms, jaicov_neq_create_timings(ENG(h), v, 8), v, 8);
}
JNIEXPORT jint JNICALL NAT(setProfiling)(JNIEnv *e, jclass k, jlong h, jboolean on) { (void)e; (void)k; return jaicov_neq_set_profiling(ENG(h), on ? 1 : 0); }
JNIEXPORT jint JNICALL NAT(kernelStats)(JNIEnv *e, jclass k, jlong h, jdoubleArray stats, jboolean reset) {
    (void)k;
    double v[16] = {0};
    return put_doubles(e, stats, jaicov_neq_kernel_stats(ENG(h), v, 16, reset ? 1 : 0), v, 16);
}
/* PDF:285-445 for the image points [begin, begin + count): w has 2 count entries, A 2 count (12 + JAICOV_MAX_DIST_PER_CAMERA) */
JNIEXPORT jint JNICALL NAT(getRows)(JNIEnv *e, jclass k, jlong h, jint begin, jint count, jdoubleArray w, jdoubleArray A) {
    (void)k;
    if (count < 0 || (*e)->GetArrayLength(e, w) < 2 * count ||
        (*e)->GetArrayLength(e, A) < 2 * count * (12 + JAICOV_MAX_DIST_PER_CAMERA)) return JAICOV_ERR_BAD_ARGUMENT;
    double *pw = (double *)(*e)->GetDoubleArrayElements(e, w, NULL);          /* small: a copy, so that only ONE array is pinned */
    if (!pw) return JAICOV_ERR_OUT_OF_MEMORY;
    double *pA = (double *)(*e)->GetPrimitiveArrayCritical(e, A, NULL);
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (pA) {
        rc = jaicov_neq_get_rows(ENG(h), (int32_t)begin, (int32_t)count, pw, pA);
        (*e)->ReleasePrimitiveArrayCritical(e, A, pA, 0);
    }
    (*e)->ReleaseDoubleArrayElements(e, w, pw, 0);
    return rc;
}
JNIEXPORT jint JNICALL NAT(getBlockWeight)(JNIEnv *e, jclass k, jlong h, jint block, jdoubleArray out) {
    (void)k;
    jsize n = (*e)->GetArrayLength(e, out);
    double *p = (double *)(*e)->GetPrimitiveArrayCritical(e, out, NULL);
    if (!p) return JAICOV_ERR_OUT_OF_MEMORY;
    int rc = jaicov_neq_get_block_weight(ENG(h), (int32_t)block, p, (size_t)n);
    (*e)->ReleasePrimitiveArrayCritical(e, out, p, 0);
    return rc;
}
JNIEXPORT jint JNICALL NAT(prepareInverse)(JNIEnv *e, jclass k, jlong h, jint invert) { (void)e; (void)k; return jaicov_neq_prepare_inverse(ENG(h), (int)invert); }
JNIEXPORT jint JNICALL NAT(reducedOrder)(JNIEnv *e, jclass k, jlong h) { (void)e; (void)k; return jaicov_neq_reduced_order(ENG(h)); }
JNIEXPORT jint JNICALL NAT(cofactorOrder)(JNIEnv *e, jclass k, jlong h) { (void)e; (void)k; return jaicov_neq_cofactor_order(ENG(h)); }

/* dx arrays must hold exactly U doubles: U (U + 1) / 2 == jaicov_neq_packed_length().  Checked before anything is read. */
static int has_u_entries(JNIEnv *e, jlong h, jdoubleArray dx) {
    const size_t n = (size_t)(*e)->GetArrayLength(e, dx);
    return n * (n + 1) / 2 == jaicov_neq_packed_length(ENG(h));
}
/* The calls below block on the device (a factorisation, its possible repeat, the inverse: up to seconds).  A critical region would
 * stall every garbage collection of the JVM for that long, so the vectors travel through a malloc'd copy (U doubles: 0.14 MB at
 * config 4) with Get/SetDoubleArrayRegion instead of GetPrimitiveArrayCritical. */
JNIEXPORT jint JNICALL NAT(solve)(JNIEnv *e, jclass k, jlong h, jint invert, jdoubleArray dx) {   /* invert = JAICOV_INVERT_* = MatrixInversion (BA:65-70) */
    (void)k;
    if (!has_u_entries(e, h, dx)) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = (*e)->GetArrayLength(e, dx);
    double *p = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    if (!p) return JAICOV_ERR_OUT_OF_MEMORY;
    int rc = jaicov_neq_solve(ENG(h), (int)invert, p);
    if (rc == JAICOV_OK) (*e)->SetDoubleArrayRegion(e, dx, 0, n, p);
    free(p);
    return rc;
}
JNIEXPORT jint JNICALL NAT(omega)(JNIEnv *e, jclass k, jlong h, jdouble s2, jdoubleArray dx, jdoubleArray out) {
    (void)k;
    double om = 0.0;
    if (!has_u_entries(e, h, dx) || (*e)->GetArrayLength(e, out) < 1) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = (*e)->GetArrayLength(e, dx);
    double *p = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    if (!p) return JAICOV_ERR_OUT_OF_MEMORY;
    (*e)->GetDoubleArrayRegion(e, dx, 0, n, p);
    int rc = jaicov_neq_omega(ENG(h), s2, p, &om);
    free(p);
    (*e)->SetDoubleArrayRegion(e, out, 0, 1, &om);
    return rc;
}
JNIEXPORT jint JNICALL NAT(update)(JNIEnv *e, jclass k, jlong h, jdoubleArray dx, jdoubleArray mx) {
    (void)k;
    double m = 0.0;
    if (!has_u_entries(e, h, dx) || (*e)->GetArrayLength(e, mx) < 1) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = (*e)->GetArrayLength(e, dx);
    double *p = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    if (!p) return JAICOV_ERR_OUT_OF_MEMORY;
    (*e)->GetDoubleArrayRegion(e, dx, 0, n, p);
    int rc = jaicov_neq_update(ENG(h), p, &m);
    free(p);
    (*e)->SetDoubleArrayRegion(e, mx, 0, 1, &m);
    return rc;
}
JNIEXPORT jint JNICALL NAT(getNormal)(JNIEnv *e, jclass k, jlong h, jdoubleArray Np, jdoubleArray nv) {
    (void)k;
    jsize len = (*e)->GetArrayLength(e, Np), U = (*e)->GetArrayLength(e, nv);
    double *pn = (double *)(*e)->GetDoubleArrayElements(e, nv, NULL);        /* small: a copy, so that only ONE array is pinned */
    if (!pn) return JAICOV_ERR_OUT_OF_MEMORY;
    double *pN = (double *)(*e)->GetPrimitiveArrayCritical(e, Np, NULL);
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (pN) {
        rc = jaicov_neq_get_normal(ENG(h), pN, (size_t)len, pn, (size_t)U);
        (*e)->ReleasePrimitiveArrayCritical(e, Np, pN, 0);
    }
    (*e)->ReleaseDoubleArrayElements(e, nv, pn, 0);
    return rc;
}
JNIEXPORT jint JNICALL NAT(getCofactor)(JNIEnv *e, jclass k, jlong h, jdoubleArray q) {
    (void)k;
    jsize n = (*e)->GetArrayLength(e, q);
    double *p = (double *)(*e)->GetPrimitiveArrayCritical(e, q, NULL);
    if (!p) return JAICOV_ERR_OUT_OF_MEMORY;
    int rc = jaicov_neq_get_cofactor(ENG(h), p, (size_t)n);
    (*e)->ReleasePrimitiveArrayCritical(e, q, p, 0);
    return rc;
}
static jint sub_block(JNIEnv *e, jlong h, int scaled, jdouble scale, jintArray idx, jdoubleArray out) {
    jsize n = (*e)->GetArrayLength(e, idx);
    if ((*e)->GetArrayLength(e, out) < n * n) return JAICOV_ERR_BAD_ARGUMENT;
    jint *ip = (*e)->GetIntArrayElements(e, idx, NULL);          /* jint is int32_t; a copy (small) */
    if (!ip) return JAICOV_ERR_OUT_OF_MEMORY;
    double *p = (double *)(*e)->GetPrimitiveArrayCritical(e, out, NULL);
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (p) {
        rc = scaled ? jaicov_neq_get_dispersion_sub(ENG(h), scale, (const int32_t *)ip, (int32_t)n, p)
                    : jaicov_neq_get_cofactor_sub(ENG(h), (const int32_t *)ip, (int32_t)n, p);
        (*e)->ReleasePrimitiveArrayCritical(e, out, p, 0);
    }
    (*e)->ReleaseIntArrayElements(e, idx, ip, JNI_ABORT);
    return rc;
}
JNIEXPORT jint JNICALL NAT(getCofactorSub)(JNIEnv *e, jclass k, jlong h, jintArray idx, jdoubleArray out) {
    (void)k;
    return sub_block(e, h, 0, 1.0, idx, out);
}
JNIEXPORT jint JNICALL NAT(getDispersionSub)(JNIEnv *e, jclass k, jlong h, jdouble scale, jintArray idx, jdoubleArray out) {
    (void)k;
    return sub_block(e, h, 1, scale, idx, out);
}
/* BA.estimateModel() on the engine.  res[0..6] = state, iterations, omega, max|dx|, final lambda, seconds total, seconds last pass */
JNIEXPORT jint JNICALL NAT(estimate)(JNIEnv *e, jclass k, jlong h, jint maxIterations, jint invert, jboolean simulation,
                                      jdouble lambda0, jdouble sigma2apriori, jdoubleArray res) {
    (void)k;
    jaicov_estimate_options o;
    jaicov_estimate_result r;
    memset(&o, 0, sizeof(o));
    memset(&r, 0, sizeof(r));
    o.struct_size = sizeof(o);
    o.max_iterations = maxIterations;
    o.invert = invert;
    o.simulation = simulation ? 1 : 0;
    o.lambda0 = lambda0;
    o.sigma2apriori = sigma2apriori;
    if ((*e)->GetArrayLength(e, res) < 7) return JAICOV_ERR_BAD_ARGUMENT;
    int rc = jaicov_neq_estimate(ENG(h), &o, &r);        /* no array is pinned while the loop runs */
    jdouble v[7] = {(jdouble)r.state, (jdouble)r.iterations, r.omega, r.max_abs_dx, r.final_lambda, r.seconds_total, r.seconds_last_pass};
    (*e)->SetDoubleArrayRegion(e, res, 0, 7, v);
    return rc;
}
/* BundleAdjustment.interrupt() (BA:1455): callable from another Java thread while estimate() runs */
JNIEXPORT jint JNICALL NAT(cancel)(JNIEnv *e, jclass k, jlong h) { (void)e; (void)k; return jaicov_neq_cancel(ENG(h)); }

/* --- include/jaicov_transform.h: CoordinateTransformationExteriorOrientation.transform on the device ------------------------- */
/* the index arrays are small: copies (Get/ReleaseIntArrayElements with JNI_ABORT); count[0] = transformed points */
JNIEXPORT jint JNICALL NAT(xformRun)(JNIEnv *e, jclass k, jlong h, jintArray points, jintArray pairRef, jintArray pairSrc, jdouble sigma2,
                                      jlongArray count) {
    (void)k;
    const jsize np = (*e)->GetArrayLength(e, points), nr = (*e)->GetArrayLength(e, pairRef);
    if ((*e)->GetArrayLength(e, pairSrc) != nr || (*e)->GetArrayLength(e, count) < 1) return JAICOV_ERR_BAD_ARGUMENT;
    jint *pp = (*e)->GetIntArrayElements(e, points, NULL);
    jint *pr = pp ? (*e)->GetIntArrayElements(e, pairRef, NULL) : NULL;
    jint *ps = pr ? (*e)->GetIntArrayElements(e, pairSrc, NULL) : NULL;
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    int32_t n = 0;
    if (ps) rc = jaicov_xform_run(ENG(h), (const int32_t *)pp, (int32_t)np, (const int32_t *)pr, (const int32_t *)ps, (int32_t)nr, sigma2, &n);
    if (ps) (*e)->ReleaseIntArrayElements(e, pairSrc, ps, JNI_ABORT);
    if (pr) (*e)->ReleaseIntArrayElements(e, pairRef, pr, JNI_ABORT);
    if (pp) (*e)->ReleaseIntArrayElements(e, points, pp, JNI_ABORT);
    const jlong v = (jlong)n;
    if (rc == JAICOV_OK) (*e)->SetLongArrayRegion(e, count, 0, 1, &v);
    return rc;
}
/* xyz: 3 n doubles, ids: 3 n longs (point, src, ref) -- through malloc'd copies and Set<Type>ArrayRegion (the int ids travel as longs) */
JNIEXPORT jint JNICALL NAT(xformGetCoordinates)(JNIEnv *e, jclass k, jlong h, jdoubleArray xyz, jlongArray ids) {
    (void)k;
    const jsize m = (*e)->GetArrayLength(e, xyz);
    if (m % 3 != 0 || (*e)->GetArrayLength(e, ids) != m) return JAICOV_ERR_BAD_ARGUMENT;
    double *px = (double *)malloc(sizeof(double) * (size_t)(m > 0 ? m : 1));
    int32_t *pi = (int32_t *)malloc(sizeof(int32_t) * (size_t)(m > 0 ? m : 1));
    jlong *pl = (jlong *)malloc(sizeof(jlong) * (size_t)(m > 0 ? m : 1));
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (px && pi && pl) {
        rc = jaicov_xform_get_coordinates(ENG(h), px, pi, (int32_t)(m / 3));
        if (rc == JAICOV_OK) {
            for (jsize i = 0; i < m; i++) pl[i] = (jlong)pi[i];
            (*e)->SetDoubleArrayRegion(e, xyz, 0, m, px);
            (*e)->SetLongArrayRegion(e, ids, 0, m, pl);
        }
    }
    free(px); free(pi); free(pl);
    return rc;
}
/* the packed covariance: one device-to-host copy into the pinned array (no device compute while it is held) */
JNIEXPORT jint JNICALL NAT(xformGetCovariance)(JNIEnv *e, jclass k, jlong h, jdoubleArray packed) {
    (void)k;
    const jsize n = (*e)->GetArrayLength(e, packed);
    double *p = (double *)(*e)->GetPrimitiveArrayCritical(e, packed, NULL);
    if (!p) return JAICOV_ERR_OUT_OF_MEMORY;
    int rc = jaicov_xform_get_covariance(ENG(h), p, (size_t)n);
    (*e)->ReleasePrimitiveArrayCritical(e, packed, p, 0);
    return rc;
}
JNIEXPORT jint JNICALL NAT(xformGetCovarianceSub)(JNIEnv *e, jclass k, jlong h, jintArray rows, jdoubleArray out) {
    (void)k;
    const jsize n = (*e)->GetArrayLength(e, rows);
    if ((*e)->GetArrayLength(e, out) < n * n) return JAICOV_ERR_BAD_ARGUMENT;
    jint *ip = (*e)->GetIntArrayElements(e, rows, NULL);
    if (!ip) return JAICOV_ERR_OUT_OF_MEMORY;
    double *p = (double *)(*e)->GetPrimitiveArrayCritical(e, out, NULL);
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (p) {
        rc = jaicov_xform_get_covariance_sub(ENG(h), (const int32_t *)ip, (int32_t)n, p);
        (*e)->ReleasePrimitiveArrayCritical(e, out, p, 0);
    }
    (*e)->ReleaseIntArrayElements(e, rows, ip, JNI_ABORT);
    return rc;
}
JNIEXPORT jint JNICALL NAT(xformGetPointBlocks)(JNIEnv *e, jclass k, jlong h, jdoubleArray out) {
    (void)k;
    const jsize m = (*e)->GetArrayLength(e, out);
    if (m % 9 != 0) return JAICOV_ERR_BAD_ARGUMENT;
    double *p = (double *)(*e)->GetPrimitiveArrayCritical(e, out, NULL);
    if (!p) return JAICOV_ERR_OUT_OF_MEMORY;
    int rc = jaicov_xform_get_point_blocks(ENG(h), p, (int32_t)(m / 9));
    (*e)->ReleasePrimitiveArrayCritical(e, out, p, 0);
    return rc;
}
JNIEXPORT jint JNICALL NAT(xformRelease)(JNIEnv *e, jclass k, jlong h) { (void)e; (void)k; return jaicov_xform_release(ENG(h)); }

/* --- include/jaicov_reliability.h: residuals, redundancy numbers and test values of every observation ------------------------- */
/* dx (null = a zero step, else exactly U doubles) is copied out of the array before the run; count[0] = observation rows */
JNIEXPORT jint JNICALL NAT(relRun)(JNIEnv *e, jclass k, jlong h, jdouble sigma2Test, jdoubleArray dx, jlongArray count) {
    (void)k;
    if ((*e)->GetArrayLength(e, count) < 1) return JAICOV_ERR_BAD_ARGUMENT;
    if (dx && !has_u_entries(e, h, dx)) return JAICOV_ERR_BAD_ARGUMENT;      /* the run reads U doubles */
    double *d = NULL;
    if (dx) {
        const jsize n = (*e)->GetArrayLength(e, dx);
        d = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
        if (!d) return JAICOV_ERR_OUT_OF_MEMORY;
        double *p = (double *)(*e)->GetPrimitiveArrayCritical(e, dx, NULL);
        if (!p) { free(d); return JAICOV_ERR_OUT_OF_MEMORY; }
        memcpy(d, p, sizeof(double) * (size_t)n);
        (*e)->ReleasePrimitiveArrayCritical(e, dx, p, JNI_ABORT);
    }
    int32_t n = 0;
    const int rc = jaicov_rel_run(ENG(h), sigma2Test, d, &n);
    free(d);
    const jlong v = (jlong)n;
    if (rc == JAICOV_OK) (*e)->SetLongArrayRegion(e, count, 0, 1, &v);
    return rc;
}
/* v, qvv, r, t (each may be null, else at least n long) through malloc'd copies and SetDoubleArrayRegion */
JNIEXPORT jint JNICALL NAT(relGet)(JNIEnv *e, jclass k, jlong h, jint n, jdoubleArray v, jdoubleArray qvv, jdoubleArray r, jdoubleArray t) {
    (void)k;
    jdoubleArray arr[4] = {v, qvv, r, t};
    double *buf[4] = {NULL, NULL, NULL, NULL};
    int rc = n < 0 ? JAICOV_ERR_BAD_ARGUMENT : JAICOV_OK;
    for (int i = 0; i < 4 && rc == JAICOV_OK; i++) {
        if (!arr[i]) continue;
        if ((*e)->GetArrayLength(e, arr[i]) < n) rc = JAICOV_ERR_BAD_ARGUMENT;
        else if (!(buf[i] = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1)))) rc = JAICOV_ERR_OUT_OF_MEMORY;
    }
    if (rc == JAICOV_OK) rc = jaicov_rel_get(ENG(h), buf[0], buf[1], buf[2], buf[3], (int32_t)n);
    for (int i = 0; i < 4; i++) {
        if (rc == JAICOV_OK && buf[i]) (*e)->SetDoubleArrayRegion(e, arr[i], 0, n, buf[i]);
        free(buf[i]);
    }
    return rc;
}
JNIEXPORT jint JNICALL NAT(relSummary)(JNIEnv *e, jclass k, jlong h, jdoubleArray out) {
    (void)k;
    if ((*e)->GetArrayLength(e, out) < 6) return JAICOV_ERR_BAD_ARGUMENT;
    double s[6];
    const int rc = jaicov_rel_summary(ENG(h), s, 6);
    if (rc == JAICOV_OK) (*e)->SetDoubleArrayRegion(e, out, 0, 6, s);
    return rc;
}
JNIEXPORT jint JNICALL NAT(relRelease)(JNIEnv *e, jclass k, jlong h) { (void)e; (void)k; return jaicov_rel_release(ENG(h)); }

/* --- include/jaicov_datum.h: the cofactor matrix re-expressed in another datum (S-transformation) ------------------------------ */
/* pointDatum: one int per object point (nonzero = datum point; the stub jni.h and the binding test know no byte[] natives), read
 * through a GetIntArrayElements copy (JNI_ABORT) into the byte mask of the C ABI; the engine checks the count against the problem's */
JNIEXPORT jint JNICALL NAT(datumTransform)(JNIEnv *e, jclass k, jlong h, jintArray pointDatum) {
    (void)k;
    if (!pointDatum) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = (*e)->GetArrayLength(e, pointDatum);
    uint8_t *mask = (uint8_t *)malloc((size_t)(n > 0 ? n : 1));
    if (!mask) return JAICOV_ERR_OUT_OF_MEMORY;
    jint *p = (*e)->GetIntArrayElements(e, pointDatum, NULL);
    if (!p) { free(mask); return JAICOV_ERR_OUT_OF_MEMORY; }
    for (jsize i = 0; i < n; i++) mask[i] = p[i] != 0;
    (*e)->ReleaseIntArrayElements(e, pointDatum, p, JNI_ABORT);
    const int rc = jaicov_datum_transform(ENG(h), mask, (int32_t)n);
    free(mask);
    return rc;
}
/* out = S v (v and out at least n long, n = cofactorOrder()) through malloc'd copies and SetDoubleArrayRegion */
JNIEXPORT jint JNICALL NAT(datumApply)(JNIEnv *e, jclass k, jlong h, jdoubleArray v, jdoubleArray out, jint n) {
    (void)k;
    if (n < 0 || !v || !out || (*e)->GetArrayLength(e, v) < n || (*e)->GetArrayLength(e, out) < n) return JAICOV_ERR_BAD_ARGUMENT;
    double *buf = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    if (!buf) return JAICOV_ERR_OUT_OF_MEMORY;
    double *p = (double *)(*e)->GetDoubleArrayElements(e, v, NULL);
    if (!p) { free(buf); return JAICOV_ERR_OUT_OF_MEMORY; }
    memcpy(buf, p, sizeof(double) * (size_t)n);
    (*e)->ReleaseDoubleArrayElements(e, v, p, JNI_ABORT);
    const int rc = jaicov_datum_apply(ENG(h), buf, buf, (int32_t)n);
    if (rc == JAICOV_OK) (*e)->SetDoubleArrayRegion(e, out, 0, n, buf);
    free(buf);
    return rc;
}

/* --- include/jaicov_dlt.h: DirectLinearTransformation.adjust for a batch of images (no engine) ---------------------------------- */
/* the inputs are read through Get<Type>ArrayElements copies (JNI_ABORT); out comes back through SetDoubleArrayRegion, status and
 * solves through long[] (the stub jni.h has no SetIntArrayRegion).  ioFixed (int[], nonzero = fixed) may be null (all free). */
JNIEXPORT jint JNICALL NAT(dltAdjust)(JNIEnv *e, jclass k, jintArray obsBegin, jdoubleArray xy, jdoubleArray xyz, jdoubleArray io,
                                      jintArray ioFixed, jintArray restrictions, jint maxIterations, jdoubleArray out, jlongArray status,
                                      jlongArray solves) {
    (void)k;
    const jsize nb = (*e)->GetArrayLength(e, obsBegin);
    if (nb < 1) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = nb - 1, nr = (*e)->GetArrayLength(e, restrictions);
    if ((*e)->GetArrayLength(e, io) < 3 * n || (ioFixed && (*e)->GetArrayLength(e, ioFixed) < 3 * n) ||
        (*e)->GetArrayLength(e, out) < 20 * n || (*e)->GetArrayLength(e, status) < n || (*e)->GetArrayLength(e, solves) < n)
        return JAICOV_ERR_BAD_ARGUMENT;
    jint *pb = (*e)->GetIntArrayElements(e, obsBegin, NULL);
    if (!pb) return JAICOV_ERR_OUT_OF_MEMORY;
    const jint nobs = pb[n];
    if (nobs < 0 || (*e)->GetArrayLength(e, xy) < 2 * nobs || (*e)->GetArrayLength(e, xyz) < 3 * nobs) {
        (*e)->ReleaseIntArrayElements(e, obsBegin, pb, JNI_ABORT);
        return JAICOV_ERR_BAD_ARGUMENT;
    }
    jdouble *pxy = (*e)->GetDoubleArrayElements(e, xy, NULL);
    jdouble *pxyz = pxy ? (*e)->GetDoubleArrayElements(e, xyz, NULL) : NULL;
    jdouble *pio = pxyz ? (*e)->GetDoubleArrayElements(e, io, NULL) : NULL;
    jint *pfx = (pio && ioFixed) ? (*e)->GetIntArrayElements(e, ioFixed, NULL) : NULL;
    jint *prs = pio ? (*e)->GetIntArrayElements(e, restrictions, NULL) : NULL;
    double *po = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? 20 * n : 1));
    int32_t *ps = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n > 0 ? 2 * n : 2));
    jlong *pl = (jlong *)malloc(sizeof(jlong) * (size_t)(n > 0 ? n : 1));
    uint8_t *pf = (uint8_t *)malloc((size_t)(n > 0 ? 3 * n : 1));
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (prs && (pfx || !ioFixed) && po && ps && pl && pf) {
        if (pfx)
            for (jsize i = 0; i < 3 * n; i++) pf[i] = pfx[i] != 0;
        rc = jaicov_dlt_adjust((int32_t)n, (const int32_t *)pb, pxy, pxyz, pio, pfx ? pf : NULL, (const int32_t *)prs, (int32_t)nr,
                               (int32_t)maxIterations, po, ps, ps + n, NULL);
        if (rc == JAICOV_OK) {
            (*e)->SetDoubleArrayRegion(e, out, 0, 20 * n, po);
            for (jsize i = 0; i < n; i++) pl[i] = (jlong)ps[i];
            (*e)->SetLongArrayRegion(e, status, 0, n, pl);
            for (jsize i = 0; i < n; i++) pl[i] = (jlong)ps[n + i];
            (*e)->SetLongArrayRegion(e, solves, 0, n, pl);
        }
    }
    free(po); free(ps); free(pl); free(pf);
    if (prs) (*e)->ReleaseIntArrayElements(e, restrictions, prs, JNI_ABORT);
    if (pfx) (*e)->ReleaseIntArrayElements(e, ioFixed, pfx, JNI_ABORT);
    if (pio) (*e)->ReleaseDoubleArrayElements(e, io, pio, JNI_ABORT);
    if (pxyz) (*e)->ReleaseDoubleArrayElements(e, xyz, pxyz, JNI_ABORT);
    if (pxy) (*e)->ReleaseDoubleArrayElements(e, xy, pxy, JNI_ABORT);
    (*e)->ReleaseIntArrayElements(e, obsBegin, pb, JNI_ABORT);
    return rc;
}

/* --- include/jaicov_intersect.h: forward intersection of a batch of object points (no engine) ----------------------------------- */
/* inputs through Get<Type>ArrayElements copies (JNI_ABORT); var, iterations, rayUsed and rayQ may be null; status, iterations and
 * rayUsed come back through long[] as for the DLT. */
JNIEXPORT jint JNICALL NAT(isectPoints)(JNIEnv *e, jclass k, jintArray rayBegin, jintArray rayImage, jdoubleArray xy, jdoubleArray var,
                                        jint nImages, jdoubleArray imageIo, jdoubleArray imageEo, jdouble sigma2apriori, jint maxIterations,
                                        jdouble rejectThreshold, jint minRays, jdoubleArray out, jlongArray status, jlongArray iterations,
                                        jlongArray rayUsed, jdoubleArray rayQ) {
    (void)k;
    const jsize nb = (*e)->GetArrayLength(e, rayBegin);
    if (nb < 1 || nImages < 0) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = nb - 1;
    if ((*e)->GetArrayLength(e, imageIo) < 3 * nImages || (*e)->GetArrayLength(e, imageEo) < 6 * nImages ||
        (*e)->GetArrayLength(e, out) < JAICOV_ISECT_OUT_PER_POINT * n || (*e)->GetArrayLength(e, status) < n ||
        (iterations && (*e)->GetArrayLength(e, iterations) < n))
        return JAICOV_ERR_BAD_ARGUMENT;
    jint *pb = (*e)->GetIntArrayElements(e, rayBegin, NULL);
    if (!pb) return JAICOV_ERR_OUT_OF_MEMORY;
    const jint nr = pb[n];
    if (nr < 0 || (*e)->GetArrayLength(e, rayImage) < nr || (*e)->GetArrayLength(e, xy) < 2 * nr ||
        (var && (*e)->GetArrayLength(e, var) < 3 * nr) || (rayUsed && (*e)->GetArrayLength(e, rayUsed) < nr) ||
        (rayQ && (*e)->GetArrayLength(e, rayQ) < nr)) {
        (*e)->ReleaseIntArrayElements(e, rayBegin, pb, JNI_ABORT);
        return JAICOV_ERR_BAD_ARGUMENT;
    }
    jint *pi = (*e)->GetIntArrayElements(e, rayImage, NULL);
    jdouble *pxy = pi ? (*e)->GetDoubleArrayElements(e, xy, NULL) : NULL;
    jdouble *pvar = (pxy && var) ? (*e)->GetDoubleArrayElements(e, var, NULL) : NULL;
    jdouble *pio = pxy ? (*e)->GetDoubleArrayElements(e, imageIo, NULL) : NULL;
    jdouble *peo = pio ? (*e)->GetDoubleArrayElements(e, imageEo, NULL) : NULL;
    const size_t np1 = (size_t)(n > 0 ? n : 1), nr1 = (size_t)(nr > 0 ? nr : 1), nl = np1 > nr1 ? np1 : nr1;
    double *po = (double *)malloc(sizeof(double) * JAICOV_ISECT_OUT_PER_POINT * np1);
    int32_t *ps = (int32_t *)malloc(sizeof(int32_t) * 2 * np1);
    uint8_t *pu = (uint8_t *)malloc(nr1);
    double *pq = (double *)malloc(sizeof(double) * nr1);
    jlong *pl = (jlong *)malloc(sizeof(jlong) * nl);
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (peo && (pvar || !var) && po && ps && pu && pq && pl) {
        rc = jaicov_isect_points((int32_t)n, (const int32_t *)pb, (const int32_t *)pi, pxy, pvar, (int32_t)nImages, pio, peo, sigma2apriori,
                                 (int32_t)maxIterations, rejectThreshold, (int32_t)minRays, po, ps, ps + n, pu, pq, NULL);
        if (rc == JAICOV_OK) {
            (*e)->SetDoubleArrayRegion(e, out, 0, JAICOV_ISECT_OUT_PER_POINT * n, po);
            for (jsize i = 0; i < n; i++) pl[i] = (jlong)ps[i];
            (*e)->SetLongArrayRegion(e, status, 0, n, pl);
            if (iterations) {
                for (jsize i = 0; i < n; i++) pl[i] = (jlong)ps[n + i];
                (*e)->SetLongArrayRegion(e, iterations, 0, n, pl);
            }
            if (rayUsed) {
                for (jsize i = 0; i < nr; i++) pl[i] = (jlong)pu[i];
                (*e)->SetLongArrayRegion(e, rayUsed, 0, nr, pl);
            }
            if (rayQ) (*e)->SetDoubleArrayRegion(e, rayQ, 0, nr, pq);
        }
    }
    free(po); free(ps); free(pu); free(pq); free(pl);
    if (peo) (*e)->ReleaseDoubleArrayElements(e, imageEo, peo, JNI_ABORT);
    if (pio) (*e)->ReleaseDoubleArrayElements(e, imageIo, pio, JNI_ABORT);
    if (pvar) (*e)->ReleaseDoubleArrayElements(e, var, pvar, JNI_ABORT);
    if (pxy) (*e)->ReleaseDoubleArrayElements(e, xy, pxy, JNI_ABORT);
    if (pi) (*e)->ReleaseIntArrayElements(e, rayImage, pi, JNI_ABORT);
    (*e)->ReleaseIntArrayElements(e, rayBegin, pb, JNI_ABORT);
    return rc;
}

/* --- include/jaicov_resect.h: spatial resection of a batch of images (no engine) -------------------------------------------------- */
/* inputs through Get<Type>ArrayElements copies (JNI_ABORT); var, eoStart, iterations, startKind, obsUsed and obsQ may be null; status,
 * iterations, startKind and obsUsed come back through long[] as for the intersection. */
JNIEXPORT jint JNICALL NAT(resectImages)(JNIEnv *e, jclass k, jintArray obsBegin, jdoubleArray xy, jdoubleArray xyz, jdoubleArray var,
                                         jdoubleArray imageIo, jdoubleArray eoStart, jdouble sigma2apriori, jint maxIterations,
                                         jdouble rejectThreshold, jint minPoints, jdoubleArray out, jlongArray status, jlongArray iterations,
                                         jlongArray startKind, jlongArray obsUsed, jdoubleArray obsQ) {
    (void)k;
    const jsize nb = (*e)->GetArrayLength(e, obsBegin);
    if (nb < 1) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = nb - 1;
    if ((*e)->GetArrayLength(e, imageIo) < 3 * n || (eoStart && (*e)->GetArrayLength(e, eoStart) < 6 * n) ||
        (*e)->GetArrayLength(e, out) < JAICOV_RESECT_OUT_PER_IMAGE * n || (*e)->GetArrayLength(e, status) < n ||
        (iterations && (*e)->GetArrayLength(e, iterations) < n) || (startKind && (*e)->GetArrayLength(e, startKind) < n))
        return JAICOV_ERR_BAD_ARGUMENT;
    jint *pb = (*e)->GetIntArrayElements(e, obsBegin, NULL);
    if (!pb) return JAICOV_ERR_OUT_OF_MEMORY;
    const jint no = pb[n];
    if (no < 0 || (*e)->GetArrayLength(e, xy) < 2 * no || (*e)->GetArrayLength(e, xyz) < 3 * no ||
        (var && (*e)->GetArrayLength(e, var) < 3 * no) || (obsUsed && (*e)->GetArrayLength(e, obsUsed) < no) ||
        (obsQ && (*e)->GetArrayLength(e, obsQ) < no)) {
        (*e)->ReleaseIntArrayElements(e, obsBegin, pb, JNI_ABORT);
        return JAICOV_ERR_BAD_ARGUMENT;
    }
    jdouble *pxy = (*e)->GetDoubleArrayElements(e, xy, NULL);
    jdouble *pxyz = pxy ? (*e)->GetDoubleArrayElements(e, xyz, NULL) : NULL;
    jdouble *pvar = (pxyz && var) ? (*e)->GetDoubleArrayElements(e, var, NULL) : NULL;
    jdouble *pio = pxyz ? (*e)->GetDoubleArrayElements(e, imageIo, NULL) : NULL;
    jdouble *peo = (pio && eoStart) ? (*e)->GetDoubleArrayElements(e, eoStart, NULL) : NULL;
    const size_t ni1 = (size_t)(n > 0 ? n : 1), no1 = (size_t)(no > 0 ? no : 1), nl = ni1 > no1 ? ni1 : no1;
    double *po = (double *)malloc(sizeof(double) * JAICOV_RESECT_OUT_PER_IMAGE * ni1);
    int32_t *ps = (int32_t *)malloc(sizeof(int32_t) * 3 * ni1);
    uint8_t *pu = (uint8_t *)malloc(no1);
    double *pq = (double *)malloc(sizeof(double) * no1);
    jlong *pl = (jlong *)malloc(sizeof(jlong) * nl);
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (pio && (pvar || !var) && (peo || !eoStart) && po && ps && pu && pq && pl) {
        rc = jaicov_resect_images((int32_t)n, (const int32_t *)pb, pxy, pxyz, pvar, pio, peo, sigma2apriori, (int32_t)maxIterations,
                                  rejectThreshold, (int32_t)minPoints, po, ps, ps + n, ps + 2 * n, pu, pq, NULL);
        if (rc == JAICOV_OK) {
            (*e)->SetDoubleArrayRegion(e, out, 0, JAICOV_RESECT_OUT_PER_IMAGE * n, po);
            jlongArray dst[3] = {status, iterations, startKind};
            for (int a = 0; a < 3; a++) {
                if (!dst[a]) continue;
                for (jsize i = 0; i < n; i++) pl[i] = (jlong)ps[(size_t)a * n + i];
                (*e)->SetLongArrayRegion(e, dst[a], 0, n, pl);
            }
            if (obsUsed) {
                for (jsize i = 0; i < no; i++) pl[i] = (jlong)pu[i];
                (*e)->SetLongArrayRegion(e, obsUsed, 0, no, pl);
            }
            if (obsQ) (*e)->SetDoubleArrayRegion(e, obsQ, 0, no, pq);
        }
    }
    free(po); free(ps); free(pu); free(pq); free(pl);
    if (peo) (*e)->ReleaseDoubleArrayElements(e, eoStart, peo, JNI_ABORT);
    if (pio) (*e)->ReleaseDoubleArrayElements(e, imageIo, pio, JNI_ABORT);
    if (pvar) (*e)->ReleaseDoubleArrayElements(e, var, pvar, JNI_ABORT);
    if (pxyz) (*e)->ReleaseDoubleArrayElements(e, xyz, pxyz, JNI_ABORT);
    if (pxy) (*e)->ReleaseDoubleArrayElements(e, xy, pxy, JNI_ABORT);
    (*e)->ReleaseIntArrayElements(e, obsBegin, pb, JNI_ABORT);
    return rc;
}

/* --- include/jaicov_relorient.h: relative orientation of a batch of image pairs (no engine) ---------------------------------------- */
/* inputs through Get<Type>ArrayElements copies (JNI_ABORT); varA, varB, start, iterations, startKind, obsUsed and obsQ may be null; status,
 * iterations, startKind and obsUsed come back through long[] as for the resection. */
JNIEXPORT jint JNICALL NAT(orientPairs)(JNIEnv *e, jclass k, jintArray obsBegin, jdoubleArray xyA, jdoubleArray xyB, jdoubleArray varA,
                                        jdoubleArray varB, jdoubleArray pairIo, jdoubleArray start, jdouble sigma2apriori, jint maxIterations,
                                        jdouble rejectThreshold, jint minPoints, jdoubleArray out, jlongArray status, jlongArray iterations,
                                        jlongArray startKind, jlongArray obsUsed, jdoubleArray obsQ) {
    (void)k;
    const jsize nb = (*e)->GetArrayLength(e, obsBegin);
    if (nb < 1) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = nb - 1;
    if ((*e)->GetArrayLength(e, pairIo) < 6 * n || (start && (*e)->GetArrayLength(e, start) < 6 * n) ||
        (*e)->GetArrayLength(e, out) < JAICOV_RELOR_OUT_PER_PAIR * n || (*e)->GetArrayLength(e, status) < n ||
        (iterations && (*e)->GetArrayLength(e, iterations) < n) || (startKind && (*e)->GetArrayLength(e, startKind) < n))
        return JAICOV_ERR_BAD_ARGUMENT;
    jint *pb = (*e)->GetIntArrayElements(e, obsBegin, NULL);
    if (!pb) return JAICOV_ERR_OUT_OF_MEMORY;
    const jint no = pb[n];
    if (no < 0 || (*e)->GetArrayLength(e, xyA) < 2 * no || (*e)->GetArrayLength(e, xyB) < 2 * no ||
        (varA && (*e)->GetArrayLength(e, varA) < 3 * no) || (varB && (*e)->GetArrayLength(e, varB) < 3 * no) ||
        (obsUsed && (*e)->GetArrayLength(e, obsUsed) < no) || (obsQ && (*e)->GetArrayLength(e, obsQ) < no)) {
        (*e)->ReleaseIntArrayElements(e, obsBegin, pb, JNI_ABORT);
        return JAICOV_ERR_BAD_ARGUMENT;
    }
    jdouble *pxa = (*e)->GetDoubleArrayElements(e, xyA, NULL);
    jdouble *pxb = pxa ? (*e)->GetDoubleArrayElements(e, xyB, NULL) : NULL;
    jdouble *pva = (pxb && varA) ? (*e)->GetDoubleArrayElements(e, varA, NULL) : NULL;
    jdouble *pvb = (pxb && varB) ? (*e)->GetDoubleArrayElements(e, varB, NULL) : NULL;
    jdouble *pio = pxb ? (*e)->GetDoubleArrayElements(e, pairIo, NULL) : NULL;
    jdouble *pst = (pio && start) ? (*e)->GetDoubleArrayElements(e, start, NULL) : NULL;
    const size_t np1 = (size_t)(n > 0 ? n : 1), no1 = (size_t)(no > 0 ? no : 1), nl = np1 > no1 ? np1 : no1;
    double *po = (double *)malloc(sizeof(double) * JAICOV_RELOR_OUT_PER_PAIR * np1);
    int32_t *ps = (int32_t *)malloc(sizeof(int32_t) * 3 * np1);
    uint8_t *pu = (uint8_t *)malloc(no1);
    double *pq = (double *)malloc(sizeof(double) * no1);
    jlong *pl = (jlong *)malloc(sizeof(jlong) * nl);
    int rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (pio && (pva || !varA) && (pvb || !varB) && (pst || !start) && po && ps && pu && pq && pl) {
        rc = jaicov_relorient_pairs((int32_t)n, (const int32_t *)pb, pxa, pxb, pva, pvb, pio, pst, sigma2apriori, (int32_t)maxIterations,
                                    rejectThreshold, (int32_t)minPoints, po, ps, ps + n, ps + 2 * n, pu, pq, NULL);
        if (rc == JAICOV_OK) {
            (*e)->SetDoubleArrayRegion(e, out, 0, JAICOV_RELOR_OUT_PER_PAIR * n, po);
            jlongArray dst[3] = {status, iterations, startKind};
            for (int a = 0; a < 3; a++) {
                if (!dst[a]) continue;
                for (jsize i = 0; i < n; i++) pl[i] = (jlong)ps[(size_t)a * n + i];
                (*e)->SetLongArrayRegion(e, dst[a], 0, n, pl);
            }
            if (obsUsed) {
                for (jsize i = 0; i < no; i++) pl[i] = (jlong)pu[i];
                (*e)->SetLongArrayRegion(e, obsUsed, 0, no, pl);
            }
            if (obsQ) (*e)->SetDoubleArrayRegion(e, obsQ, 0, no, pq);
        }
    }
    free(po); free(ps); free(pu); free(pq); free(pl);
    if (pst) (*e)->ReleaseDoubleArrayElements(e, start, pst, JNI_ABORT);
    if (pio) (*e)->ReleaseDoubleArrayElements(e, pairIo, pio, JNI_ABORT);
    if (pvb) (*e)->ReleaseDoubleArrayElements(e, varB, pvb, JNI_ABORT);
    if (pva) (*e)->ReleaseDoubleArrayElements(e, varA, pva, JNI_ABORT);
    if (pxb) (*e)->ReleaseDoubleArrayElements(e, xyB, pxb, JNI_ABORT);
    if (pxa) (*e)->ReleaseDoubleArrayElements(e, xyA, pxa, JNI_ABORT);
    (*e)->ReleaseIntArrayElements(e, obsBegin, pb, JNI_ABORT);
    return rc;
}

/* --- include/jaicov_simil.h: absolute orientation of a batch of models, and the move into the target frame (no engine) -------------- */
/* an optional double[] of at least `need` values: its copy, or NULL where the array is null; *bad is set where it is too short or the
 * copy failed */
static jdouble *simil_get(JNIEnv *e, jdoubleArray a, jsize need, int *bad) {
    if (!a) return NULL;
    if ((*e)->GetArrayLength(e, a) < need) { *bad = JAICOV_ERR_BAD_ARGUMENT; return NULL; }
    jdouble *p = (*e)->GetDoubleArrayElements(e, a, NULL);
    if (!p && !*bad) *bad = JAICOV_ERR_OUT_OF_MEMORY;
    return p;
}

/* inputs through Get<Type>ArrayElements copies (JNI_ABORT); cofSrc, cofDst, start, iterations, startKind, ptUsed and ptQ may be null;
 * status, iterations, startKind and ptUsed come back through long[] as for the relative orientation. */
JNIEXPORT jint JNICALL NAT(similModels)(JNIEnv *e, jclass k, jintArray ptBegin, jdoubleArray src, jdoubleArray dst, jdoubleArray cofSrc,
                                        jdoubleArray cofDst, jdoubleArray start, jint maxIterations, jdouble rejectThreshold, jint minPoints,
                                        jdoubleArray out, jlongArray status, jlongArray iterations, jlongArray startKind, jlongArray ptUsed,
                                        jdoubleArray ptQ) {
    (void)k;
    if (!ptBegin || !src || !dst || !out || !status) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize nb = (*e)->GetArrayLength(e, ptBegin);
    if (nb < 1) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = nb - 1;
    if ((*e)->GetArrayLength(e, out) < JAICOV_SIMIL_OUT_PER_MODEL * n || (*e)->GetArrayLength(e, status) < n ||
        (iterations && (*e)->GetArrayLength(e, iterations) < n) || (startKind && (*e)->GetArrayLength(e, startKind) < n))
        return JAICOV_ERR_BAD_ARGUMENT;
    jint *pb = (*e)->GetIntArrayElements(e, ptBegin, NULL);
    if (!pb) return JAICOV_ERR_OUT_OF_MEMORY;
    const jint np = pb[n];
    if (np < 0 || (ptUsed && (*e)->GetArrayLength(e, ptUsed) < np) || (ptQ && (*e)->GetArrayLength(e, ptQ) < np)) {
        (*e)->ReleaseIntArrayElements(e, ptBegin, pb, JNI_ABORT);
        return JAICOV_ERR_BAD_ARGUMENT;
    }
    int rc = 0;
    jdouble *ps = simil_get(e, src, 3 * np, &rc), *pd = simil_get(e, dst, 3 * np, &rc), *pqs = simil_get(e, cofSrc, 6 * np, &rc);
    jdouble *pqd = simil_get(e, cofDst, 6 * np, &rc), *pst = simil_get(e, start, 7 * n, &rc);
    const size_t nm1 = (size_t)(n > 0 ? n : 1), np1 = (size_t)(np > 0 ? np : 1), nl = nm1 > np1 ? nm1 : np1;
    double *po = (double *)malloc(sizeof(double) * JAICOV_SIMIL_OUT_PER_MODEL * nm1);
    int32_t *pc = (int32_t *)malloc(sizeof(int32_t) * 3 * nm1);
    uint8_t *pu = (uint8_t *)malloc(np1);
    double *pq = (double *)malloc(sizeof(double) * np1);
    jlong *pl = (jlong *)malloc(sizeof(jlong) * nl);
    if (!rc && !(po && pc && pu && pq && pl)) rc = JAICOV_ERR_OUT_OF_MEMORY;
    if (!rc) {
        rc = jaicov_simil_models((int32_t)n, (const int32_t *)pb, ps, pd, pqs, pqd, pst, (int32_t)maxIterations, rejectThreshold,
                                 (int32_t)minPoints, po, pc, pc + n, pc + 2 * n, pu, pq, NULL);
        if (rc == JAICOV_OK) {
            (*e)->SetDoubleArrayRegion(e, out, 0, JAICOV_SIMIL_OUT_PER_MODEL * n, po);
            jlongArray to[3] = {status, iterations, startKind};
            for (int a = 0; a < 3; a++) {
                if (!to[a]) continue;
                for (jsize i = 0; i < n; i++) pl[i] = (jlong)pc[(size_t)a * n + i];
                (*e)->SetLongArrayRegion(e, to[a], 0, n, pl);
            }
            if (ptUsed) {
                for (jsize i = 0; i < np; i++) pl[i] = (jlong)pu[i];
                (*e)->SetLongArrayRegion(e, ptUsed, 0, np, pl);
            }
            if (ptQ) (*e)->SetDoubleArrayRegion(e, ptQ, 0, np, pq);
        }
    }
    free(po); free(pc); free(pu); free(pq); free(pl);
    if (pst) (*e)->ReleaseDoubleArrayElements(e, start, pst, JNI_ABORT);
    if (pqd) (*e)->ReleaseDoubleArrayElements(e, cofDst, pqd, JNI_ABORT);
    if (pqs) (*e)->ReleaseDoubleArrayElements(e, cofSrc, pqs, JNI_ABORT);
    if (pd) (*e)->ReleaseDoubleArrayElements(e, dst, pd, JNI_ABORT);
    if (ps) (*e)->ReleaseDoubleArrayElements(e, src, ps, JNI_ABORT);
    (*e)->ReleaseIntArrayElements(e, ptBegin, pb, JNI_ABORT);
    return rc;
}

/* ptBegin with xyz, cof, xyzOut, cofOut, and imgBegin with eo, eoOut, may be null; the outputs are written through scratch buffers */
JNIEXPORT jint JNICALL NAT(similApply)(JNIEnv *e, jclass k, jdoubleArray par, jintArray ptBegin, jdoubleArray xyz, jdoubleArray cof,
                                       jintArray imgBegin, jdoubleArray eo, jdoubleArray xyzOut, jdoubleArray cofOut, jdoubleArray eoOut) {
    (void)k;
    if (!par || (*e)->GetArrayLength(e, par) % 7 || (cof == NULL) != (cofOut == NULL)) return JAICOV_ERR_BAD_ARGUMENT;
    const jsize n = (*e)->GetArrayLength(e, par) / 7;
    if ((ptBegin && (*e)->GetArrayLength(e, ptBegin) != n + 1) || (imgBegin && (*e)->GetArrayLength(e, imgBegin) != n + 1) ||
        (ptBegin && (!xyz || !xyzOut)) || (imgBegin && (!eo || !eoOut)))
        return JAICOV_ERR_BAD_ARGUMENT;
    jint *pb = ptBegin ? (*e)->GetIntArrayElements(e, ptBegin, NULL) : NULL;
    jint *ib = imgBegin ? (*e)->GetIntArrayElements(e, imgBegin, NULL) : NULL;
    int rc = ((ptBegin && !pb) || (imgBegin && !ib)) ? JAICOV_ERR_OUT_OF_MEMORY : 0;
    const jint np = (!rc && pb) ? pb[n] : 0, ni = (!rc && ib) ? ib[n] : 0;
    if (!rc && (np < 0 || ni < 0 || (np > 0 && (*e)->GetArrayLength(e, xyzOut) < 3 * np) || (np > 0 && cofOut && (*e)->GetArrayLength(e, cofOut) < 6 * np) ||
                (ni > 0 && (*e)->GetArrayLength(e, eoOut) < 6 * ni)))
        rc = JAICOV_ERR_BAD_ARGUMENT;
    jdouble *pp = NULL, *px = NULL, *pq = NULL, *pe = NULL;
    double *ox = NULL, *oq = NULL, *oe = NULL;
    if (!rc) {
        pp = simil_get(e, par, 7 * n, &rc);
        px = np > 0 ? simil_get(e, xyz, 3 * np, &rc) : NULL;
        pq = np > 0 ? simil_get(e, cof, 6 * np, &rc) : NULL;
        pe = ni > 0 ? simil_get(e, eo, 6 * ni, &rc) : NULL;
        ox = (double *)malloc(sizeof(double) * 3 * (size_t)(np > 0 ? np : 1));
        oq = (double *)malloc(sizeof(double) * 6 * (size_t)(np > 0 ? np : 1));
        oe = (double *)malloc(sizeof(double) * 6 * (size_t)(ni > 0 ? ni : 1));
        if (!rc && !(ox && oq && oe)) rc = JAICOV_ERR_OUT_OF_MEMORY;
    }
    if (!rc) {
        rc = jaicov_simil_apply((int32_t)n, pp, np > 0 ? (const int32_t *)pb : NULL, px, pq, ni > 0 ? (const int32_t *)ib : NULL, pe, ox,
                                pq ? oq : NULL, oe);
        if (rc == JAICOV_OK) {
            if (np > 0) (*e)->SetDoubleArrayRegion(e, xyzOut, 0, 3 * np, ox);
            if (np > 0 && pq) (*e)->SetDoubleArrayRegion(e, cofOut, 0, 6 * np, oq);
            if (ni > 0) (*e)->SetDoubleArrayRegion(e, eoOut, 0, 6 * ni, oe);
        }
    }
    free(ox); free(oq); free(oe);
    if (pe) (*e)->ReleaseDoubleArrayElements(e, eo, pe, JNI_ABORT);
    if (pq) (*e)->ReleaseDoubleArrayElements(e, cof, pq, JNI_ABORT);
    if (px) (*e)->ReleaseDoubleArrayElements(e, xyz, px, JNI_ABORT);
    if (pp) (*e)->ReleaseDoubleArrayElements(e, par, pp, JNI_ABORT);
    if (ib) (*e)->ReleaseIntArrayElements(e, imgBegin, ib, JNI_ABORT);
    if (pb) (*e)->ReleaseIntArrayElements(e, ptBegin, pb, JNI_ABORT);
    return rc;
}
