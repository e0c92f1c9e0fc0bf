/* qdisc_ref: drives the reference's own socket queues (network_queuing_disciplines.c over
 * priority_queue.c, compiled in place from a reference checkout) with offer / select scripts.
 *
 * What is the reference's compiled code here: the heap, its comparator, the round-robin queue.
 * What this file restates, by line and in its own words:
 *   host/descriptor/socket.c:198-199,437-442,466-467   a socket is a control FIFO and a data FIFO; a
 *       packet of priority 0 enters the control FIFO; the next packet is the control head if any
 *   host/network/network_interface.c:344-370   wantsSend: a socket that is not found in the queue is
 *       pushed as a fresh reference, one that is found is left alone
 *   host/network/network_interface.c:205-294   one selection step: pop a socket, pull its packet,
 *       push the socket back if it has more and is not found in the queue, else drop the reference
 * As in the reference, the queues hold references (small boxes naming a socket), not sockets:
 * equality and hash go by the socket a reference names, and every reference is dropped once.
 *
 * Input (stdin), any number of scripts:
 *   <qdisc> <nsockets>      0 = fifo (heap), 1 = round robin
 *   o <slot> <prio> <tag>   the packet enters the socket, then wantsSend
 *   s                       one selection step; prints "<slot> <tag>", or "-" on an empty queue
 *   e                       ends the script (so does the end of input); prints "e"
 * Everything is freed through the queues' own destroy functions, so the program is clean under
 * ASan / UBSan with no options set.  Exit status 2 on a malformed script. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "main/host/network/network_queuing_disciplines.h"

typedef struct {
    uint64_t prio, tag;
} Pkt;

typedef struct {
    Pkt* items;
    size_t head, count, capacity;
} Fifo;

typedef struct {
    unsigned slot;
    Fifo control, data;
} Sock;

struct InetSocket {
    Sock* sock;
};

static long live_refs = 0; /* references made and not yet dropped; 0 at the end of a script */

static void fifo_push(Fifo* f, Pkt p) {
    if (f->head + f->count == f->capacity) {
        if (f->head > 0) {
            memmove(f->items, f->items + f->head, f->count * sizeof(Pkt));
            f->head = 0;
        } else {
            f->capacity = f->capacity ? 2 * f->capacity : 4;
            f->items = realloc(f->items, f->capacity * sizeof(Pkt));
            if (!f->items) {
                abort();
            }
        }
    }
    f->items[f->head + f->count++] = p;
}

static Pkt fifo_pop(Fifo* f) {
    Pkt p = f->items[f->head++];
    if (--f->count == 0) {
        f->head = 0;
    }
    return p;
}

/* ---- the socket side (socket.c, restated) and the bindings the queues call */
static void sock_add(Sock* s, Pkt p) { fifo_push(p.prio == 0 ? &s->control : &s->data, p); }
static bool sock_has_data(const Sock* s) { return s->control.count + s->data.count > 0; }
static const Fifo* sock_next_fifo(const Sock* s) { return s->control.count ? &s->control : &s->data; }

static const InetSocket* ref_clone(const InetSocket* r) {
    InetSocket* c = malloc(sizeof *c);
    if (!c) {
        abort();
    }
    c->sock = r->sock;
    live_refs++;
    return c;
}

void inetsocket_drop(const InetSocket* socket) {
    live_refs--;
    free((void*)socket);
}

bool inetsocket_eqVoid(const void* a, const void* b) {
    return ((const InetSocket*)a)->sock == ((const InetSocket*)b)->sock;
}

/* slots 16 apart share a cell of a small table: the table's probing is exercised */
unsigned int inetsocket_hashVoid(const void* socket) { return ((const InetSocket*)socket)->sock->slot % 16u * 7u; }

int inetsocket_peekNextPacketPriority(const InetSocket* socket, uint64_t* priority_out) {
    const Sock* s = socket->sock;
    if (!sock_has_data(s)) {
        return -1;
    }
    const Fifo* f = sock_next_fifo(s);
    *priority_out = f->items[f->head].prio;
    return 0;
}

/* ---- the interface side (network_interface.c, restated) over either queue */
typedef struct {
    int qdisc;
    RrSocketQueue rr;
    FifoSocketQueue fifo;
} Interface;

static bool q_empty(Interface* i) { return i->qdisc ? rrsocketqueue_isEmpty(&i->rr) : fifosocketqueue_isEmpty(&i->fifo); }
static bool q_find(Interface* i, const InetSocket* s) {
    return i->qdisc ? rrsocketqueue_find(&i->rr, s) : fifosocketqueue_find(&i->fifo, s);
}
static void q_push(Interface* i, const InetSocket* s) {
    if (i->qdisc) {
        rrsocketqueue_push(&i->rr, s);
    } else {
        fifosocketqueue_push(&i->fifo, s);
    }
}
static bool q_pop(Interface* i, InetSocket** s) {
    return i->qdisc ? rrsocketqueue_pop(&i->rr, s) : fifosocketqueue_pop(&i->fifo, s);
}

static void wants_send(Interface* i, const InetSocket* s) {
    if (!sock_has_data(s->sock)) {
        return;
    }
    if (!q_find(i, s)) {
        q_push(i, ref_clone(s));
    }
}

static bool select_one(Interface* i, unsigned* slot, uint64_t* tag) {
    while (!q_empty(i)) {
        InetSocket* s = NULL;
        if (!q_pop(i, &s)) {
            continue;
        }
        Sock* sock = s->sock;
        if (!sock_has_data(sock)) {
            inetsocket_drop(s);
            continue;
        }
        Pkt p = fifo_pop(sock->control.count ? &sock->control : &sock->data);
        if (sock_has_data(sock) && !q_find(i, s)) {
            q_push(i, s);
        } else {
            inetsocket_drop(s);
        }
        *slot = sock->slot;
        *tag = p.tag;
        return true;
    }
    return false;
}

/* the queues' own destroy functions drop what is still queued */
static void teardown(Interface* i, Sock* socks, InetSocket* handles, unsigned nsockets) {
    if (i->qdisc) {
        rrsocketqueue_destroy(&i->rr, inetsocket_drop);
    } else {
        fifosocketqueue_destroy(&i->fifo, inetsocket_drop);
    }
    for (unsigned k = 0; k < nsockets; k++) {
        free(socks[k].control.items);
        free(socks[k].data.items);
    }
    free(socks);
    free(handles);
}

static int bad(const char* what, long line) {
    fprintf(stderr, "qdisc_ref: line %ld: %s\n", line, what);
    return 2;
}

int main(void) {
    char buf[256];
    long line = 0;
    int rc = 0;
    Interface itf;
    Sock* socks = NULL;
    InetSocket* handles = NULL; /* the callers' own references, one per socket, never queued */
    unsigned nsockets = 0;
    bool open = false;

    while (rc == 0) {
        char* got = fgets(buf, sizeof buf, stdin);
        line++;
        bool end = !got || buf[0] == 'e';
        if (end && open) {
            teardown(&itf, socks, handles, nsockets);
            socks = NULL;
            handles = NULL;
            open = false;
            if (live_refs != 0) {
                rc = bad("a socket reference was not dropped exactly once", line);
            }
            if (got) {
                puts("e");
            }
        }
        if (!got) {
            break;
        }
        if (end || buf[0] == '\n') {
            continue;
        }
        if (!open) {
            int qdisc;
            if (sscanf(buf, "%d %u", &qdisc, &nsockets) != 2 || (qdisc != 0 && qdisc != 1) || nsockets == 0) {
                rc = bad("expected '<qdisc 0|1> <nsockets>'", line);
                break;
            }
            memset(&itf, 0, sizeof itf);
            itf.qdisc = qdisc;
            if (qdisc) {
                rrsocketqueue_init(&itf.rr);
            } else {
                fifosocketqueue_init(&itf.fifo);
            }
            socks = calloc(nsockets, sizeof *socks);
            handles = calloc(nsockets, sizeof *handles);
            if (!socks || !handles) {
                abort();
            }
            for (unsigned k = 0; k < nsockets; k++) {
                socks[k].slot = k;
                handles[k].sock = &socks[k];
            }
            open = true;
        } else if (buf[0] == 'o') {
            unsigned slot;
            Pkt p;
            if (sscanf(buf + 1, "%u %" SCNu64 " %" SCNu64, &slot, &p.prio, &p.tag) != 3 || slot >= nsockets) {
                rc = bad("expected 'o <slot> <prio> <tag>' with slot < nsockets", line);
                break;
            }
            sock_add(&socks[slot], p);
            wants_send(&itf, &handles[slot]);
        } else if (buf[0] == 's') {
            unsigned slot;
            uint64_t tag;
            if (select_one(&itf, &slot, &tag)) {
                printf("%u %" PRIu64 "\n", slot, tag);
            } else {
                puts("-");
            }
        } else {
            rc = bad("unknown op", line);
        }
    }
    if (open) { /* left by an error: still free everything */
        teardown(&itf, socks, handles, nsockets);
    }
    return rc;
}
