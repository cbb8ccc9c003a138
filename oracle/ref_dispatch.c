/* oracle/ref_dispatch.c -- a driver for the reference's own dispatcher.  TEST INFRASTRUCTURE ONLY.
 *
 * oracle/Makefile links this file with the reference's rpc_server_skeleton.c,
 * rpc_server_helpers.c, rpc_server_impl.c and cJSON.c, compiled in place (the source list of
 * the reference's server minus its main), into oracle/_ref/ref_dispatch.  No socket, no CRC
 * library and no GPU: bodies in, the dispatcher's strings out.
 *
 *   stdin:   per body    a 32-bit little-endian length, then that many bytes
 *   stdout:  per body    a 32-bit little-endian length, then the returned string without its
 *                        NUL; the length 0xFFFFFFFF alone when the dispatcher returned NULL
 *
 * Each body is handed over followed by a 0 byte, as the reference's server hands over what it
 * read from the wire: the dispatcher sees a C string, so a body with a 0 byte inside ends
 * there for it.  Exit status 0 at a clean end of input, 1 on a cut record or a failed
 * allocation or write. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

char* rpc_server_dispatch(const char* req_json); /* the reference's, from its skeleton */

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
        char* reply = rpc_server_dispatch(body);
        int ok;
        if (reply == NULL) {
            ok = put_u32(stdout, 0xFFFFFFFFu);
        } else {
            size_t n = strlen(reply);
            ok = n < 0xFFFFFFFFu && put_u32(stdout, (uint32_t)n) && fwrite(reply, 1, n, stdout) == n;
            free(reply);
        }
        if (!ok) {
            free(body);
            return 1;
        }
    }
    free(body);
    return more == 0 && fflush(stdout) == 0 ? 0 : 1;
}
