// a5x_rules_nest.hip -- k_rules_stream<the seven nested algorithms, a5x_nest.h>: the kernel
// of a5x_rules.hip instantiated in a translation unit of its own (see the note above
// a5x_launch_rules_stream there).
#define A5X_RULES_NEST 1
#include "a5x_rules.hip"
