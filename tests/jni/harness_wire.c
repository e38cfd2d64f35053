/*
 * harness_wire.c -- TEST INFRASTRUCTURE: the entry points of libjniharness.so for the shim's natives of the segment in
 * channel bytes (blockSumsSegmentWire, matchScanSegmentWire).  As harness_tokens.c includes harness.c, this file
 * includes harness_tokens.c: the library is built from this translation unit, has every jh_* entry point of both
 * unchanged, and adds nothing to the JNIEnv -- the two natives use only functions harness.c already implements.
 */
#include "harness_tokens.c"

void NC(blockSumsSegmentWire)(JNIEnv*, jclass, jlongArray, jobjectArray, jintArray, jlongArray, jintArray, jbyteArray,
                              jobjectArray, jlongArray);
jlongArray NC(matchScanSegmentWire)(JNIEnv*, jclass, jlongArray, jobjectArray, jintArray, jlongArray, jintArray,
                                    jobjectArray, jlongArray, jbyteArray, jobjectArray, jbyteArray, jlongArray);

/* The device set the natives take: jh_set_multi's contexts, or the one context (0: a closed one). */
#define CTXS(ctx)                                                  \
    jlong one_ctx = (ctx);                                         \
    fobj cs_o = {K_LONG, g_nmulti ? g_multi : &one_ctx, g_nmulti ? g_nmulti : 1}; \
    jobject cs = &cs_o

/* A ByteBuffer[] of n buffers, bufs[i] with caps[i] (< 0: a heap buffer; NULL with cap 0: a Java null). */
static void buffer_array(fobj* store, jobject* refs, void** bufs, const jlong* caps, int n) {
    buffers(store, refs, bufs, caps, n);
    for (int i = 0; i < n; ++i)
        if (!bufs[i] && caps[i] == 0) refs[i] = NULL;
}

/* bufs / caps: the nb data buffers; wire / wire_caps: one output buffer per file; wire_len: nf longs out. */
JNIEXPORT void jh_block_sums_segment_wire(jlong ctx, void** bufs, const jlong* caps, int nb, int32_t* file_pieces, int nf,
                                          jlong* sizes, int32_t* hdrs, uint8_t* seed, void** wire,
                                          const jlong* wire_caps, jlong* wire_len, jlong wire_len_n) {
    reset();
    fobj* store = (fobj*)calloc((size_t)nb + 1, sizeof(fobj));
    jobject* refs = (jobject*)calloc((size_t)nb + 1, sizeof(jobject));
    buffers(store, refs, bufs, caps, nb);
    fobj arr = {K_OBJS, refs, nb};
    fobj* ws = (fobj*)calloc((size_t)nf + 1, sizeof(fobj));
    jobject* wr = (jobject*)calloc((size_t)nf + 1, sizeof(jobject));
    buffer_array(ws, wr, wire, wire_caps, nf);
    fobj wa = {K_OBJS, wr, nf};
    OBJ(fp, K_INT, file_pieces, nf);
    OBJ(sz, K_LONG, sizes, nf);
    OBJ(h, K_INT, hdrs, 4 * nf);
    OBJ(s, K_BYTE, seed, 4);
    OBJ(wl, K_LONG, wire_len, wire_len_n);
    CTXS(ctx);
    NC(blockSumsSegmentWire)(&g_env, NULL, cs, &arr, fp, sz, h, s, &wa, wl);
    free(refs);
    free(store);
    free(ws);
    free(wr);
}

/* tables / table_caps / table_lens: one record buffer per file; replies / reply_caps: one output buffer per file;
 * per_file: 5 longs per file out.  Returns the event longs' count (-1: the native returned null). */
JNIEXPORT jlong jh_match_scan_segment_wire(jlong ctx, void** bufs, const jlong* caps, int nb, int32_t* file_pieces,
                                           int nf, jlong* sizes, int32_t* hdrs, void** tables, const jlong* table_caps,
                                           jlong* table_lens, uint8_t* seed, void** replies, const jlong* reply_caps,
                                           uint8_t* md5, jlong md5_len, jlong* per_file, jlong per_len, jlong* ev_out,
                                           jlong ev_cap) {
    reset();
    fobj* store = (fobj*)calloc((size_t)nb + 1, sizeof(fobj));
    jobject* refs = (jobject*)calloc((size_t)nb + 1, sizeof(jobject));
    buffers(store, refs, bufs, caps, nb);
    fobj arr = {K_OBJS, refs, nb};
    fobj* ts = (fobj*)calloc((size_t)nf + 1, sizeof(fobj));
    jobject* tr = (jobject*)calloc((size_t)nf + 1, sizeof(jobject));
    fobj* rs = (fobj*)calloc((size_t)nf + 1, sizeof(fobj));
    jobject* rr = (jobject*)calloc((size_t)nf + 1, sizeof(jobject));
    buffer_array(ts, tr, tables, table_caps, nf);
    buffer_array(rs, rr, replies, reply_caps, nf);
    fobj ta = {K_OBJS, tr, nf}, ra = {K_OBJS, rr, nf};
    OBJ(fp, K_INT, file_pieces, nf);
    OBJ(sz, K_LONG, sizes, nf);
    OBJ(h, K_INT, hdrs, 4 * nf);
    OBJ(tl, K_LONG, table_lens, nf);
    OBJ(s, K_BYTE, seed, 4);
    OBJ(m, K_BYTE, md5, md5_len);
    OBJ(pf, K_LONG, per_file, per_len);
    CTXS(ctx);
    jlong r = events_back(NC(matchScanSegmentWire)(&g_env, NULL, cs, &arr, fp, sz, h, &ta, tl, s, &ra, m, pf), ev_out,
                          ev_cap);
    free(refs);
    free(store);
    free(ts);
    free(tr);
    free(rs);
    free(rr);
    return r;
}
