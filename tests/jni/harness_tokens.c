/*
 * harness_tokens.c -- TEST INFRASTRUCTURE: the entry points of libjniharness.so for the shim's tokensKept native
 * (and ctxTrim, which its test needs).  harness.c keeps its fake JNIEnv file-local, so this file includes it -- the
 * library is built from this translation unit and has every jh_* entry point of harness.c unchanged -- and adds
 * nothing to the JNIEnv: tokensKept uses only functions harness.c already implements.
 */
#include "harness.c"

jboolean NC(tokensKept)(JNIEnv*, jclass, jlong, jlongArray, jint, jbyteArray, jlong, jobject, jlong);
void NC(ctxTrim)(JNIEnv*, jclass, jlong);

/* events: events_len longs (a Java null when events_len < 0 with a NULL pointer); out: a direct buffer of out_cap
 * bytes (out_cap < 0: a heap buffer).  Returns the native's boolean. */
JNIEXPORT int jh_tokens_kept(jlong ctx, jlong* events, jlong events_len, int n_ev, uint8_t* md5, jlong md5_len,
                             jlong from, void* out, jlong out_cap, jlong len) {
    reset();
    OBJ(e, K_LONG, events, events_len);
    OBJ(m, K_BYTE, md5, md5_len);
    BUF(o, out, out_cap);
    return NC(tokensKept)(&g_env, NULL, ctx, e, n_ev, m, from, o, len);
}

JNIEXPORT void jh_ctx_trim(jlong ctx) {
    reset();
    NC(ctxTrim)(&g_env, NULL, ctx);
}
