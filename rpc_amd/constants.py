"""The constants of include/rpccrc.h and of the reference's rpc.h that the package exports."""

# reference rpc.h:11-17
RPC_TYPE_DATA = 0
RPC_TYPE_PING = 1
RPC_TYPE_PONG = 2
RPC_HEADER_LEN = 12
MAX_BODY_LEN = 1024

# frame verdicts and flags (include/rpccrc.h RPC_FRAME_* / RPC_FRAMES_*)
FRAME_BAD_CRC = 0
FRAME_OK = 1
FRAME_CONTROL = 2
FRAME_TOO_LARGE = 3
FRAME_MALFORMED = 4
FRAME_RECV_ERR = 5  # client role, body_len 0: rpc_async.c:330-349 drops the connection (RPC_RECV_ERR)
FRAME_NOT_REACHED = 6  # frames_scan(verify=True): behind a frame that closed its connection
FRAME_SKIPPED = 7  # frames_pack: the caller asked for no frame here (TYPE_NONE)
TYPE_NONE = 0xFFFF  # frames_pack: a type value meaning "emit nothing for this entry"
CONN_OPEN = 0
CONN_CLOSED = 1
FRAMES_SERVER = 0x1
FRAMES_CLIENT = 0x2
FRAMES_LIFT_CAP = 0x4
# frames_carry (include/rpccrc.h RPC_FRAMES_CARRY_ROOM / RPC_CARRY_*)
CARRY_ROOM = 1040  # >= 12 + MAX_BODY_LEN - 1, a multiple of 16: any tail with the cap in force
CARRY_OK = 0
CARRY_CLOSED = 1
CARRY_INVALID = 2
CARRY_NO_ROOM = 3
# frames_route (include/rpccrc.h RPC_ROUTE_*)
ROUTE_NONE = 0
ROUTE_CALL = 1
ROUTE_NOT_FOUND = 2
ROUTE_INVALID = 3
ROUTE_DEFER = 4
ROUTE_RANGE = 5
ROUTE_NO_METHOD = 0xFFFF
ROUTE_MAX_BODY = 1024
ROUTE_MAX_DEPTH = 32
ROUTE_MAX_TOKENS = 256
ROUTE_MAX_METHODS = 256
ROUTE_MAX_METHOD_BYTES = 4096
# frames_args (include/rpccrc.h RPC_ARGS_* / RPC_ARG_*)
ARGS_NONE = 0
ARGS_OK = 1
ARGS_INVALID = 2
ARGS_DEFER = 3
ARGS_RANGE = 4
ARGS_BAD_SCHEMA = 5
ARG_I32 = 0
ARG_I64 = 1
ARG_F64 = 2
ARG_BOOL = 3
ARG_STR = 4
ARGS_MAX_PARAMS = 8
ARGS_MAX_SCHEMA_PARAMS = 1024
ARGS_MAX_NAME_BYTES = 4096
# frames_resolve (include/rpccrc.h RPC_RESOLVE_*)
RESOLVE_NONE = 0
RESOLVE_MATCHED = 1
RESOLVE_UNKNOWN = 2
RESOLVE_DUPLICATE = 3
RESOLVE_INVALID = 4
RESOLVE_DEFER = 5
RESOLVE_RANGE = 6
RESOLVE_NO_SLOT = 0xFFFFFFFF
RESOLVE_MAX_PENDING = 1 << 24
# frames_reply (include/rpccrc.h RPC_REPLY_*)
REPLY_NONE = 0
REPLY_RESULT = 1
REPLY_ERROR = 2
REPLY_RAW = 3
REPLY_RANGE = 4
REPLY_NO_ROOM = 5
# frames_request (include/rpccrc.h RPC_REQUEST_*)
REQUEST_NONE = 0
REQUEST_CALL = 1
REQUEST_RAW = 2
REQUEST_BAD_METHOD = 3
REQUEST_RANGE = 4
REQUEST_NO_ROOM = 5
# frames_values (include/rpccrc.h RPC_VALUES_*)
VALUES_NONE = 0
VALUES_OK = 1
VALUES_TEXT = 2
VALUES_DEFER = 3
VALUES_RANGE = 4
VALUES_BAD_SCHEMA = 5
VALUES_NO_ROOM = 6
VALUES_MODE_NONE = 0
VALUES_MODE_ENCODE = 1
VALUES_MODE_TEXT = 2
VALUES_FORM_RESULT = 0
VALUES_FORM_PARAMS = 1
