/* The glib functions declared in shim/glib.h: a linear-probe hash table and a ring of pointers.
 * Both hold at most a host's sockets, so neither is tuned. */
#include <glib.h>

#include <stdio.h>
#include <string.h>

gpointer shim_alloc(gsize bytes) {
    gpointer p = malloc(bytes ? bytes : 1);
    if (!p) {
        fprintf(stderr, "qdisc_ref: out of memory\n");
        abort();
    }
    return p;
}

gpointer shim_realloc(gpointer mem, gsize bytes) {
    gpointer p = realloc(mem, bytes ? bytes : 1);
    if (!p) {
        fprintf(stderr, "qdisc_ref: out of memory\n");
        abort();
    }
    return p;
}

/* ---- GHashTable: open addressing, linear probing, deletion by re-inserting the run behind the
 * freed cell (no tombstones).  `used` cells hold live entries; the table is at most half full. */
typedef struct {
    gpointer key, value;
    int used;
} Cell;

struct _GHashTable {
    GHashFunc hash;
    GEqualFunc equal;
    Cell* cells;
    gsize capacity, count; /* capacity is a power of two */
};

static void table_alloc(GHashTable* t, gsize capacity) {
    t->cells = shim_alloc(sizeof(Cell) * capacity);
    memset(t->cells, 0, sizeof(Cell) * capacity);
    t->capacity = capacity;
    t->count = 0;
}

/* the cell that holds `key`, or the free cell where it would go */
static Cell* table_probe(GHashTable* t, gconstpointer key) {
    gsize i = (gsize)t->hash(key) & (t->capacity - 1);
    while (t->cells[i].used && !t->equal(t->cells[i].key, key)) {
        i = (i + 1) & (t->capacity - 1);
    }
    return &t->cells[i];
}

static void table_grow(GHashTable* t) {
    Cell* old = t->cells;
    gsize old_capacity = t->capacity;
    table_alloc(t, old_capacity * 2);
    for (gsize i = 0; i < old_capacity; i++) {
        if (old[i].used) {
            Cell* c = table_probe(t, old[i].key);
            *c = old[i];
            t->count++;
        }
    }
    free(old);
}

GHashTable* g_hash_table_new(GHashFunc hash_func, GEqualFunc key_equal_func) {
    GHashTable* t = shim_alloc(sizeof(GHashTable));
    t->hash = hash_func;
    t->equal = key_equal_func;
    table_alloc(t, 16);
    return t;
}

void g_hash_table_destroy(GHashTable* table) {
    free(table->cells);
    free(table);
}

gboolean g_hash_table_insert(GHashTable* table, gpointer key, gpointer value) {
    Cell* c = table_probe(table, key);
    if (c->used) {
        c->value = value; /* the present key stays, as in glib */
        return FALSE;
    }
    if ((table->count + 1) * 2 > table->capacity) {
        table_grow(table);
        c = table_probe(table, key);
    }
    c->key = key;
    c->value = value;
    c->used = 1;
    table->count++;
    return TRUE;
}

gpointer g_hash_table_lookup(GHashTable* table, gconstpointer key) {
    Cell* c = table_probe(table, key);
    return c->used ? c->value : NULL;
}

gboolean g_hash_table_remove(GHashTable* table, gconstpointer key) {
    Cell* c = table_probe(table, key);
    if (!c->used) {
        return FALSE;
    }
    c->used = 0;
    table->count--;
    /* every entry of the run behind the freed cell is taken out and put in again */
    gsize i = ((gsize)(c - table->cells) + 1) & (table->capacity - 1);
    while (table->cells[i].used) {
        Cell moved = table->cells[i];
        table->cells[i].used = 0;
        *table_probe(table, moved.key) = moved;
        i = (i + 1) & (table->capacity - 1);
    }
    return TRUE;
}

void g_hash_table_remove_all(GHashTable* table) {
    memset(table->cells, 0, sizeof(Cell) * table->capacity);
    table->count = 0;
}

/* ---- GQueue: a ring of GList cells that doubles when full */
struct _GQueue {
    GList* cells;
    gsize capacity, head, count;
};

GQueue* g_queue_new(void) {
    GQueue* q = shim_alloc(sizeof(GQueue));
    q->capacity = 8;
    q->cells = shim_alloc(sizeof(GList) * q->capacity);
    q->head = q->count = 0;
    return q;
}

void g_queue_free(GQueue* queue) {
    free(queue->cells);
    free(queue);
}

gboolean g_queue_is_empty(GQueue* queue) { return queue->count == 0; }

gpointer g_queue_pop_head(GQueue* queue) {
    if (queue->count == 0) {
        return NULL;
    }
    gpointer data = queue->cells[queue->head].data;
    queue->head = (queue->head + 1) % queue->capacity;
    queue->count--;
    return data;
}

void g_queue_push_tail(GQueue* queue, gpointer data) {
    if (queue->count == queue->capacity) {
        GList* bigger = shim_alloc(sizeof(GList) * queue->capacity * 2);
        for (gsize k = 0; k < queue->count; k++) {
            bigger[k] = queue->cells[(queue->head + k) % queue->capacity];
        }
        free(queue->cells);
        queue->cells = bigger;
        queue->capacity *= 2;
        queue->head = 0;
    }
    queue->cells[(queue->head + queue->count) % queue->capacity].data = data;
    queue->count++;
}

/* glib: the first element for which func(element, data) is 0 */
GList* g_queue_find_custom(GQueue* queue, gconstpointer data, GCompareFunc func) {
    for (gsize k = 0; k < queue->count; k++) {
        GList* cell = &queue->cells[(queue->head + k) % queue->capacity];
        if (func(cell->data, data) == 0) {
            return cell;
        }
    }
    return NULL;
}
