/* tests/dropin/ref_encode.c -- a driver for the reference client's request encoder.  TEST
 * INFRASTRUCTURE ONLY.
 *
 * tests/request_ref.py links this file with the reference's client/rpc_codec.c and
 * third_party/cJSON.c, compiled in place, into a temporary directory.  No socket, no CRC library
 * and no GPU: (name, params text or none, id) in, what rpc_codec_encode_request makes of each out.
 *
 *   stdin:   per request   the name as a 32-bit little-endian length and that many bytes, the
 *                          params text likewise (the length 0xFFFFFFFF alone: no params), the id
 *                          (32-bit little-endian)
 *   stdout:  per request   cJSON_PrintUnformatted of the parsed params alone, then the encoded
 *                          request, each as a 32-bit little-endian length and that many bytes;
 *                          the length 0xFFFFFFFF alone for params that are not there or that
 *                          cJSON_Parse refused (the request is then encoded without them) and for
 *                          a request the encoder did not return
 *
 * The name and the params text are handed over followed by a 0 byte, as C strings: either ends
 * at a 0 byte inside it.  Exit status 0 at a clean end of input, 1 on a cut record or a failed
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

static int put_u32(FILE* f, uint32_t v)
{
    unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
    return fwrite(b, 1, 4, f) == 4;
}

static int put_text(FILE* f, const char* text)
{
    if (text == NULL) {
        return put_u32(f, 0xFFFFFFFFu);
    }
    size_t n = strlen(text);
    return n < 0xFFFFFFFFu && put_u32(f, (uint32_t)n) && fwrite(text, 1, n, f) == n;
}

/* A length-prefixed string as a fresh C string; *none is set for the length 0xFFFFFFFF. */
static char* get_text(FILE* f, int* none)
{
    uint32_t len;
    *none = 0;
    if (get_u32(f, &len) != 1) {
        return NULL;
    }
    if (len == 0xFFFFFFFFu) {
        *none = 1;
        len = 0;
    }
    char* s = (char*)malloc((size_t)len + 1);
    if (s == NULL || fread(s, 1, len, f) != len) {
        free(s);
        return NULL;
    }
    s[len] = '\0';
    return s;
}

int main(void)
{
    for (;;) {
        uint32_t name_len;
        int more = get_u32(stdin, &name_len);
        if (more != 1) {
            return more == 0 && fflush(stdout) == 0 ? 0 : 1;
        }
        char* name = (char*)malloc((size_t)name_len + 1);
        if (name == NULL || fread(name, 1, name_len, stdin) != name_len) {
            free(name);
            return 1;
        }
        name[name_len] = '\0';
        int none = 0;
        uint32_t id = 0;
        char* text = get_text(stdin, &none);
        if (text == NULL || get_u32(stdin, &id) != 1) {
            free(name);
            free(text);
            return 1;
        }
        cJSON* params = none ? NULL : cJSON_Parse(text);
        char* printed = params ? cJSON_PrintUnformatted(params) : NULL;
        char* request = rpc_codec_encode_request(name, params, id); /* (the params now belong to the request) */
        int ok = put_text(stdout, printed) && put_text(stdout, request);
        free(printed);
        free(request);
        free(text);
        free(name);
        if (!ok) {
            return 1;
        }
    }
}
