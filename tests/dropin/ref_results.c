/* tests/dropin/ref_results.c -- a driver that says what the reference's generated client would
 * read from a reply.  TEST INFRASTRUCTURE ONLY.
 *
 * tests/results_ref.py links this file with the reference's client/rpc_codec.c and
 * third_party/cJSON.c, compiled in place, into a temporary directory.  No socket, no CRC library
 * and no GPU: bodies in, the facts about the `result` node that rpc_codec_decode_response hands
 * over, and about `error`'s `code` and `message`, out.
 *
 *   stdin:   per body    a 32-bit little-endian length, then that many bytes
 *   stdout:  per body    the return code (32-bit little-endian), then three nodes -- result,
 *                        error.code, error.message -- each as: one byte "is there"; four bytes
 *                        cJSON_IsString / IsNumber / IsBool / IsTrue; the 8 bytes of valuedouble;
 *                        strtoll(valuestring, NULL, 10) as 8 bytes (0 without a string); the
 *                        length of valuestring (32 bits, 0xFFFFFFFF without one) and its bytes
 *
 * Each body is handed over followed by a 0 byte, as the reference's client hands over what it
 * read from the wire.  Exit status 0 at a clean end of input, 1 on a cut record or a failed
 * allocation or write. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rpc_codec.h"

static int get_u32(FILE* f, uint32_t* v)
{
    unsigned char b[4];
    size_t got = fread(b, 1, 4, f);
    if (got != 4) {
        return got == 0 ? 0 : -1; /* a clean end, or a cut record */
    }
    *v = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    return 1;
}

static int put_bytes(FILE* f, const void* p, size_t n)
{
    return fwrite(p, 1, n, f) == n;
}

static int put_u32(FILE* f, uint32_t v)
{
    unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
    return put_bytes(f, b, 4);
}

static int put_node(FILE* f, const cJSON* node)
{
    unsigned char flags[5] = {0, 0, 0, 0, 0};
    double d = 0.0;
    long long ll = 0;
    const char* s = NULL;
    if (node != NULL) {
        flags[0] = 1;
        flags[1] = cJSON_IsString(node) ? 1 : 0;
        flags[2] = cJSON_IsNumber(node) ? 1 : 0;
        flags[3] = cJSON_IsBool(node) ? 1 : 0;
        flags[4] = cJSON_IsTrue(node) ? 1 : 0;
        d = node->valuedouble;
        s = flags[1] ? node->valuestring : NULL;
        if (s != NULL) {
            ll = strtoll(s, NULL, 10);
        }
    }
    int64_t v = (int64_t)ll;
    if (!put_bytes(f, flags, 5) || !put_bytes(f, &d, 8) || !put_bytes(f, &v, 8)) {
        return 0;
    }
    if (s == NULL) {
        return put_u32(f, 0xFFFFFFFFu);
    }
    size_t n = strlen(s);
    return n < 0xFFFFFFFFu && put_u32(f, (uint32_t)n) && put_bytes(f, s, n);
}

int main(void)
{
    char* body = NULL;
    size_t cap = 0;
    uint32_t len;
    int more;
    while ((more = get_u32(stdin, &len)) == 1) {
        if ((size_t)len + 1 > cap) {
            char* grown = (char*)realloc(body, (size_t)len + 1);
            if (grown == NULL) {
                free(body);
                return 1;
            }
            body = grown;
            cap = (size_t)len + 1;
        }
        if (fread(body, 1, len, stdin) != len) {
            free(body);
            return 1;
        }
        body[len] = '\0';
        uint32_t id = 0;
        cJSON* result = NULL;
        cJSON* error = NULL;
        int rc = rpc_codec_decode_response(body, &id, &result, &error);
        if (rc != 0) {
            result = NULL, error = NULL;
        }
        const cJSON* code = cJSON_IsObject(error) ? cJSON_GetObjectItemCaseSensitive(error, "code") : NULL;
        const cJSON* message = cJSON_IsObject(error) ? cJSON_GetObjectItemCaseSensitive(error, "message") : NULL;
        int ok = put_u32(stdout, (uint32_t)rc) && put_node(stdout, result) && put_node(stdout, code) &&
                 put_node(stdout, message);
        cJSON_Delete(result);
        cJSON_Delete(error);
        if (!ok) {
            free(body);
            return 1;
        }
    }
    free(body);
    return more == 0 && fflush(stdout) == 0 ? 0 : 1;
}
