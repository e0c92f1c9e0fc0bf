/* Stands in for the reference's generated bindings header: the opaque socket type and the four
 * socket functions its qdisc code calls.  driver.c defines them. */
#ifndef REF_QDISC_SHIM_BINDINGS_H
#define REF_QDISC_SHIM_BINDINGS_H

#include <stdbool.h>
#include <stdint.h>

typedef struct InetSocket InetSocket;

bool inetsocket_eqVoid(const void* a, const void* b);
unsigned int inetsocket_hashVoid(const void* socket);
int inetsocket_peekNextPacketPriority(const InetSocket* socket, uint64_t* priority_out);
void inetsocket_drop(const InetSocket* socket);

#endif
