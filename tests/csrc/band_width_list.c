/* Prints the oracle's strip width of the banded sweep (decree B2: poa_band_strip_width, oracle/poa_oracle.h) for every
 * length from 1 to argv[1], one per line: tests/test_class_matrix_fixture.py holds the class matrix's model of the host's
 * choice equal to it. */
#include <stdio.h>
#include <stdlib.h>
#include "../../oracle/poa_oracle.h"

int main(int argc, char **argv) {
    const long top = argc > 1 ? atol(argv[1]) : 0;
    for (long L = 1; L <= top; ++L) printf("%d\n", poa_band_strip_width(L));
    return 0;
}
