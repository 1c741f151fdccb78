// a5x_rules_wide.hip -- k_rules_stream<SHA-224 | SHA-384 | SHA-512>: the kernel of
// a5x_rules.hip instantiated in a translation unit of its own (see the note above
// a5x_launch_rules_stream there).
#define A5X_RULES_WIDE 1
#include "a5x_rules.hip"
