/* tests/dropin/ref_decode.c -- a driver for the reference client's reply decoder.  TEST
 * INFRASTRUCTURE ONLY.
 *
 * tests/resolve_ref.py links this file with the reference's client/rpc_codec.c and
 * third_party/cJSON.c, compiled in place, into a temporary directory.  No socket, no CRC library
 * and no GPU: bodies in, what rpc_codec_decode_response says about each out.
 *
 *   stdin:   per body    a 32-bit little-endian length, then that many bytes
 *   stdout:  per body    the return code and the id (32-bit little-endian each; the id is 0
 *                        when the code is not 0), then cJSON_PrintUnformatted of *result and of
 *                        *error, each as a 32-bit little-endian length and that many bytes, the
 *                        length 0xFFFFFFFF alone for a member that is not there
 *
 * Each body is handed over followed by a 0 byte, as the reference's client hands over what it
 * read from the wire: the decoder sees a C string, so a body with a 0 byte inside ends there for
 * it.  Exit status 0 at a clean end of input, 1 on a cut record or a failed allocation or
 * write. */
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

static int put_u32(FILE* f, uint32_t v)
{
    unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
    return fwrite(b, 1, 4, f) == 4;
}

static int put_member(FILE* f, cJSON* node)
{
    if (node == NULL) {
        return put_u32(f, 0xFFFFFFFFu);
    }
    char* text = cJSON_PrintUnformatted(node);
    if (text == NULL) {
        return 0;
    }
    size_t n = strlen(text);
    int ok = n < 0xFFFFFFFFu && put_u32(f, (uint32_t)n) && fwrite(text, 1, n, f) == n;
    free(text);
    return ok;
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
            id = 0, result = NULL, error = NULL;
        }
        int ok = put_u32(stdout, (uint32_t)rc) && put_u32(stdout, id) && put_member(stdout, result) &&
                 put_member(stdout, error);
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
