// a5x_digest_nest.hip -- k_digest_stream<the seven nested algorithms, a5x_nest.h>: the kernel
// of a5x_digest.hip instantiated in a translation unit of its own (see the note above
// a5x_launch_digest_stream_nest there).
#define A5X_DIGEST_NEST 1
#include "a5x_digest.hip"
